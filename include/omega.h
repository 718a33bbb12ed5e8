/*
 * omega.h -- C ABI of libomega.so, the MI355X (gfx950) engine for the OMEGA-4 per-frame audio
 * analysis hot path: multi-resolution windowed R2C FFT + psychoacoustic weighting + interpolated
 * combine, K-weighted LUFS (zero-phase biquads), 4x true peak, the per-stream meter aggregates,
 * perceptual/mel band reductions and chromagram binning.
 *
 * Each entry point replaces one reference Python surface (reference repo paths, file:line):
 *
 *   omega_process_frames   MultiResolutionFFT.process_audio_chunk     omega4/audio/multi_resolution_fft.py:228-302
 *                          + combine_results_optimized                 multi_resolution_fft.py:335-408
 *                          + ProfessionalMetering.calculate_lufs       omega4/panels/professional_meters.py:231-281
 *                          (batched over channel-frames; the reference calls these once per display frame,
 *                           omega4_main.py:707-717 and professional_meters.py:348-351)
 *   omega_process_stream   the same over the stream layout: frame f = samples [f*hop, f*hop + W) of one
 *                          buffer per channel (the CircularBuffer.read_latest(N) view of :52-133 once
 *                          W samples have arrived)
 *   omega_combine          combine_results_optimized                   multi_resolution_fft.py:335-408
 *   omega_true_peak        ProfessionalMetering.calculate_true_peak    professional_meters.py:283-299
 *   omega_true_peak_os     calculate_true_peak(x, oversampling)         professional_meters.py:283-299
 *   omega_k_weighting      ProfessionalMetering.apply_k_weighting      professional_meters.py:129-153
 *                          (+ the instantaneous LUFS of calculate_lufs :236-246)
 *   omega_meter_*          the momentary/short-term/integrated/range/true-peak deques  professional_meters.py:19-25, :248-279
 *   omega_bands_*          AudioProcessingPipeline.map_to_bands       omega4/audio/pipeline.py:295-335 (max-reduce)
 *                          PrecomputedFrequencyMapper.map_spectrum_to_bars omega4/optimization/freq_mapper.py:165-196 (mean-reduce)
 *   omega_chroma           ChromagramAnalyzer.compute_chromagram      omega4/panels/chromagram.py:109-159
 *   omega_rfft             BatchedFFTProcessor process_batch (CPU/CuPy branches) omega4/optimization/batched_fft_processor.py:148-285
 *   omega_spectra          omega_rfft -> omega_bands_apply (MAX) + omega_chroma fused in one pass (cfg3)
 *   omega_drum_features    EnhancedKickDetector / EnhancedSnareDetector band flux, adaptive thresholds and
 *                          spectral centroid  omega4/analyzers/drum_detection.py:47-103, :212-305 (§8(f) row 1)
 *   omega_weighting        ProfessionalMetering.apply_weighting (K / A / C / Z) professional_meters.py:74-229
 *   omega_calculate_lufs   ProfessionalMetering.calculate_lufs (weighting + TP + aggregates) professional_meters.py:231-281
 *                          at scipy's float64 precision, any frame length above filtfilt's padlen
 *   omega_post_*           the app's spectrum post-processing          omega4_main.py:748-1056 (§8(f) row 2)
 *   omega_vu_*             VUMetersPanel.update ballistics             omega4/panels/vu_meters.py:55-99 (§8(f) row 2)
 *   omega_ingest_*         capture chunks -> ring -> analysis          omega4/audio/capture.py:512-600,
 *                          omega4_main.py:648-688 (§8(f) row 3)
 *   omega_transients       TransientAnalyzer.analyze_transients        omega4/analyzers/transient.py:19-108 (§8(f) row 4)
 *   omega_pitch_*          CepstralAnalyzer.detect_pitch_advanced      omega4/panels/pitch_detection.py:21-611 (§8(f) row 5)
 *   omega_harmonic_*       HarmonicAnalyzer.detect_harmonic_series     omega4/panels/harmonic_analysis.py:193-333 with
 *                          HarmonicMetrics (THD, THD+N, spectral shape, HNR, LPC formants)
 *                          omega4/analyzers/harmonic_metrics.py:51-357 (§8(f) row 6)
 *   omega_genre_*          GenreClassifier.extract_features            omega4/panels/genre_classification.py:175-422,
 *                          :600-783 (§8(f) row 7)
 *   omega_basszoom_*       BassZoomPanel.setup_bass_mapping            omega4/panels/bass_zoom.py:51-97 and
 *                          _process_bass_detail_internal               bass_zoom.py:141-232 (§8(f) row 12)
 *   omega_waterfall_*      SpectrogramWaterfall.update, _spectrum_to_color omega4/panels/spectrogram_waterfall.py:56-121,
 *                          :142-205 and SpectrogramWaterfallPanel.update  :295-305 (omega_waterfall_config_default,
 *                          _mapping, _configure, _state_size, _rows, _colors)
 *   omega_tonal_*          ChromagramAnalyzer.detect_key, get_alternative_keys, detect_chord
 *                          omega4/panels/chromagram.py:215-339, :396-418, :670-812 and MusicTheory.analyze_mode
 *                          omega4/panels/music_theory.py:175-200 (§8(f) row 13)
 *
 * Conventions:
 *   - every function returns 0 on success and a negative omega_status on error; the message is
 *     available from omega_last_error(ctx). No C++ exception and no abort crosses the ABI.
 *   - all buffers are caller-owned. `mem` says whether the data pointers are host (OMEGA_MEM_HOST:
 *     the call stages through context-owned device buffers and returns when outputs are in host
 *     memory) or device (OMEGA_MEM_DEVICE: the call enqueues on the context stream and returns
 *     immediately; synchronize with omega_synchronize).
 *   - one context per host thread (contexts own a HIP stream and the per-channel meter state);
 *     a context is not internally locked.
 *   - channel-frame index cf = f * n_channels + c; input sample n of channel-frame (f, c) lives at
 *     x[f * frame_stride + c * channel_stride + n] (materialized layout: frame_stride = C*W,
 *     channel_stride = W; stream layout with hop H over planar channels: frame_stride = H,
 *     channel_stride = samples per channel).
 */
#ifndef OMEGA_H
#define OMEGA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMEGA_ABI_VERSION 5
#define OMEGA_MAX_RES 4
#define OMEGA_N_METERS 5 /* momentary, short_term, integrated, range, true_peak */

typedef enum {
  OMEGA_OK = 0,
  OMEGA_EINVAL = -1,  /* bad argument / config (the reference raises ValueError) */
  OMEGA_EHIP = -2,    /* HIP runtime error */
  OMEGA_ENOMEM = -3,
  OMEGA_EUNSUP = -4   /* valid for the reference, not supported by this build (e.g. a batch frame size W
                         that is not a power of two 512..16384) */
} omega_status;

typedef enum { OMEGA_MEM_HOST = 0, OMEGA_MEM_DEVICE = 1 } omega_mem;

typedef enum {
  OMEGA_WIN_BLACKMAN = 0, /* np.blackman, multi_resolution_fft.py:177-178 */
  OMEGA_WIN_HANN = 1,     /* np.hanning, batched_fft_processor.py:94 */
  OMEGA_WIN_HAMMING = 2,  /* np.hamming */
  OMEGA_WIN_RECT = 3      /* ones */
} omega_window;

/* One FFT resolution: FFTConfig (multi_resolution_fft.py:26-44). */
typedef struct {
  double freq_lo, freq_hi; /* inclusive range [lo, hi] in Hz */
  int32_t fft_size;        /* power of two, 2..frame_size (below 512: mrfft_small_kernel) */
  int32_t hop_size;        /* kept for fidelity (CircularBuffer sizing); the frame API is stateless */
  double weight;           /* base psychoacoustic weight and combine weight */
  int32_t window;          /* omega_window */
} omega_resolution;

typedef struct {
  int32_t sample_rate;     /* fs */
  double max_freq;         /* combine grid top: min(max_freq, fs/2) (multi_resolution_fft.py:146) */
  int32_t n_res;           /* 1..OMEGA_MAX_RES */
  omega_resolution res[OMEGA_MAX_RES];
  int32_t apply_weighting; /* process_audio_chunk(apply_weighting=...) */
  int32_t target_bins;     /* T of combine_results_optimized, 2..4096 */
  int32_t frame_size;      /* W = metering window M: power of two 512..16384 */
  int32_t n_channels;      /* independent streams; one meter state each */
  double gate_lufs;        /* -70 (professional_meters.py:36) */
  int32_t momentary_len, short_len, integrated_len, peak_len; /* 24, 180, 3600, 60 (:20-25) */
} omega_config;

/* Per-call outputs; any pointer may be NULL to skip that stage. */
typedef struct {
  float* combined;              /* [n_cf, T] combine_results_optimized magnitude */
  float* lufs_inst;             /* [n_cf] instantaneous K-weighted LUFS (-100 when silent) */
  float* true_peak_db;          /* [n_cf] calculate_true_peak (dBTP, -100 when silent) */
  double* meters;               /* [n_cf, 5] calculate_lufs dict values; advances the meter state */
  float* mag[OMEGA_MAX_RES];    /* [n_cf, N_r/2+1] weighted magnitude per resolution (full-magnitude mode) */
  float* weighted;              /* [n_cf, W] K-weighted signal (apply_k_weighting) */
} omega_outputs;

typedef struct omega_ctx omega_ctx;

/* Reference defaults: the four resolutions of multi_resolution_fft.py:149-154, fs 48000,
 * max_freq 20000, T 1024, W 4096, one channel, gate/deques of professional_meters.py:20-36. */
void omega_config_default(omega_config* cfg);

int omega_create(const omega_config* cfg, int device, omega_ctx** out);
void omega_destroy(omega_ctx* ctx);
const char* omega_last_error(const omega_ctx* ctx);
const char* omega_version(void);
/* Enqueue on a caller-owned hipStream_t (NULL = the null/default stream, e.g. PyTorch's default
 * stream). Contexts start on a private non-blocking stream. Switching streams orders the new stream
 * (and the context's side stream) after the work already enqueued on the old one, once.
 *
 * Concurrency precondition of the default layout (omega_set_graphs): the batch kernel on this stream
 * and the meter prep on the context's side stream wait for each other through device counters, so the
 * two must be able to run at once. Each context owns two streams (its private one and the side stream;
 * a graph-capture stream only once graphs are enabled); HIP maps streams onto GPU_MAX_HW_QUEUES
 * hardware queues per process. omega_create and every stream switch here probe the pair (a waiter on
 * the side stream that must see a value stored by a kernel enqueued after it on this stream) and, on a
 * shared queue, move the side stream to a new one (the next queue), up to three times (each distinct
 * stream once; omega_check_queues re-probes). Should that fail,
 * or another tenant hold every CU, the wait is bounded (OMEGA_POLL_LIMIT polls): that call's meter
 * aggregates may be stale and OMEGA_EHIP is returned -- by the call itself for host memory, by the
 * next call or omega_synchronize for device memory. Layouts other than 0 order the side stream by
 * events and carry no such condition (but serialise on a shared queue). A stream switch synchronises
 * both streams once (the probe). */
int omega_set_stream(omega_ctx* ctx, void* hip_stream);
/* Probe the context's stream and its side stream again, whatever was probed before (a stream switch
 * probes each distinct stream once): streams created since -- an RCCL communicator's, another library's
 * -- may share a hardware queue with the side stream. Moves the side stream as omega_set_stream does
 * (and, with meter pipelining enabled, re-probes the context's two batch streams the same way);
 * *shared (optional) = 1 if no independent queue was found (the device waits then run to their bound;
 * omega_last_error says so), else 0. Synchronises both streams (a pending meter segment launches
 * first). Not part of the reference surface: the multi-GPU host calls it once its collectives exist. */
int omega_check_queues(omega_ctx* ctx, int* shared);
/* flags: bit 0 = HIP graphs: device-memory omega_process_frames calls are captured once per distinct
 * argument set and replayed afterwards (default off: measured slower than direct launches on MI355X,
 * see DESIGN.md); bits 1-2 = stream layout:
 * 0 default: 16384-sample frames on direct launches run as ONE batch kernel (K-weighting, true peak,
 * every resolution and -- up to 2048 frames per channel -- the meter aggregates as workgroup roles of
 * one grid) with the meter prep on a side stream ordered by device counters instead of stream events;
 * other calls (and graph capture) as below;
 * any other value: the full-chip kernels back to back on the stream, the latency-bound meter prep and
 * LUFS query kernels on a side stream joined by events. Every layout gives the same outputs bitwise. */
int omega_set_graphs(omega_ctx* ctx, int flags);
/* The stream calls enqueue on (omega_set_stream), and the context's configuration and device. */
void* omega_get_stream(const omega_ctx* ctx);
int omega_get_config(const omega_ctx* ctx, omega_config* cfg, int* device);
/* Waits for the work enqueued on the context's stream (a pending meter segment launched first). */
int omega_synchronize(omega_ctx* ctx);

/* Meter pipelining (default off; ABI 3). When on, a direct device-memory omega_process_frames /
 * omega_process_stream call on the default layout with meters (up to 2048 frames per channel) leaves
 * its meter aggregates (out->meters) PENDING: the next such call's one batch launch computes them
 * first in its grid -- their inputs are complete once that batch starts -- instead of this launch
 * ending with them, so consecutive calls overlap the meters of one with the transforms of the next.
 * Every other output of a call is complete when its stream work is, as always; its meters are complete
 * when the stream work of the NEXT call, omega_flush_meters or omega_synchronize is. Any other use of
 * the meter state (omega_meter_update / omega_meter_reset / omega_calculate_lufs, a host-memory,
 * graph or other-layout call, omega_set_stream, omega_set_graphs, disabling pipelining,
 * omega_destroy) launches a pending segment first, on the stream of its batch. The caller keeps the
 * pending call's meters buffer alive and unwritten until then (the segment writes it). The segment
 * and the meter prep read the batch's LUFS_inst / true-peak values from the context's own staging
 * (two sets in turn), never from the caller's lufs_inst / true_peak_db buffers, which are free to be
 * reused by the next call as soon as this call's stream work completes (they receive copies).
 * Outputs are bitwise those of the default. In this mode the batch kernel never waits for the side
 * stream (the meter prep follows it there behind a stream wait on the batch's last workgroup; only the
 * next launch's meter segment waits for the prep).
 *
 * Overlapped batches (devices with stream-wait-value support): with pipelining on, such a call's batch
 * launch and, behind it, its meter segment run on one of two streams of the context's, in turn, so the
 * drain of one call's launch runs under the start of the next. The call waits for what the caller's
 * stream holds when it is made (its input may be produced there). ALL its outputs, not only its meters,
 * are ordered into the caller's stream by the next batch call on the context, omega_flush_meters or
 * omega_synchronize (and by every call listed above that launches a pending segment), and its INPUT
 * must stay unmodified until then. A call whose input or outputs overlap the outputs of the call
 * before it, or whose outputs overlap that call's input, waits for that call first. */
int omega_set_meter_pipelining(omega_ctx* ctx, int enable);
/* Enqueue a pending meter segment now (no-op without one); complete with the stream's work. */
int omega_flush_meters(omega_ctx* ctx);

/* The fused per-channel-frame hot path over n_frames x n_channels frames of W samples. */
int omega_process_frames(omega_ctx* ctx, const float* x, int64_t n_frames, int64_t frame_stride,
                         int64_t channel_stride, const omega_outputs* out, int mem);

/* Stream layout: n_samples per channel (channel c at x + c*channel_stride), one frame per hop
 * samples once a full window has arrived: n_frames = n_samples < W ? 0 : (n_samples - W)/hop + 1,
 * frame f = x[f*hop, f*hop + W). hop must be even; *n_frames_out (may be NULL) receives the count. */
int omega_process_stream(omega_ctx* ctx, const float* x, int64_t n_samples, int32_t hop, int64_t channel_stride,
                         const omega_outputs* out, int mem, int64_t* n_frames_out);

/* combine_results_optimized over externally supplied weighted magnitudes; mags[r] may be NULL
 * (resolution absent from the results dict). out: [n_cf, T]. */
int omega_combine(omega_ctx* ctx, const float* const* mags, int64_t n_cf, float* out, int mem);

/* calculate_true_peak(x, 4) for n frames of length m (power of two 512..16384), contiguous. */
int omega_true_peak(omega_ctx* ctx, const float* x, int64_t n, int32_t m, float* out_db, int mem);
/* calculate_true_peak(x, oversampling) (professional_meters.py:283-299) for oversampling 1, 2 or 4:
 * max |resample(x, oversampling * m)| over the phases n + p / oversampling; other factors return
 * OMEGA_EUNSUP. n frames of any length m >= 1, contiguous: powers of two 512..16384 on the
 * register-FFT / Stockham kernels, every other length on the mixed-radix transform (anyfft.hip). */
int omega_true_peak_os(omega_ctx* ctx, const float* x, int64_t n, int32_t m, int32_t oversampling, float* out_db,
                       int mem);

/* apply_k_weighting for n frames of length m (power of two 512..16384): weighted [n, m] (may be
 * NULL) and the instantaneous LUFS [n] (may be NULL). */
int omega_k_weighting(omega_ctx* ctx, const float* x, int64_t n, int32_t m, float* weighted,
                      float* lufs_inst, int mem);

/* apply_weighting + instantaneous LUFS for a weighting mode (professional_meters.py:220-229):
 * K (0, :129-153), A (1, :155-192: four cascaded Butterworth filtfilt sections, x 2.5), C (2, :194-218:
 * two sections) and Z (3: the signal itself, no gate). The A and C coefficients are built for the
 * context's sample rate (create_a/c_weighting_filter, :74-127). */
typedef enum { OMEGA_WEIGHT_K = 0, OMEGA_WEIGHT_A = 1, OMEGA_WEIGHT_C = 2, OMEGA_WEIGHT_Z = 3 } omega_weighting_mode;
int omega_weighting(omega_ctx* ctx, const float* x, int64_t n, int32_t m, int32_t mode, float* weighted,
                    float* lufs_inst, int mem);

/* Meter aggregates from precomputed instantaneous values: feeds n_frames x n_channels values
 * (cf-major) through the per-channel state and writes meters [n_cf, 5]. */
int omega_meter_update(omega_ctx* ctx, const float* lufs_inst, const float* tp_db, int64_t n_frames,
                       double* meters, int mem);
int omega_meter_reset(omega_ctx* ctx);
/* The meter state of a stream whose last n_l frames had the instantaneous LUFS lufs_inst [n_l, C] and
 * whose last n_t of them (n_t <= n_l) the true peaks tp_db [n_t, C] (time order, frame-major), the next
 * frame following them: what omega_meter_reset + omega_meter_update over those n_l frames (the true
 * peaks of the n_l - n_t older ones -100 dBTP) leave, written by one kernel without computing their
 * aggregates (a time-sharded stream's rank loads the history before its shard; SURVEY §8(e),
 * omega_gpu/dist.py meter_time_shard). Rows beyond the windows (n_l > integrated_len - 1, n_t >
 * peak_len - 1) are older than anything the state keeps: the last ones are used. Replaces the reference's deques
 * (professional_meters.py:20-25) filled by calculate_lufs calls. */
int omega_meter_load_history(omega_ctx* ctx, const float* lufs_inst, int64_t n_l, const float* tp_db, int64_t n_t,
                             int mem);

/* ProfessionalMetering.calculate_lufs (professional_meters.py:231-281) in one call: weighting `mode`
 * (LUFS_inst only, as omega_weighting), calculate_true_peak(x, oversampling) (as omega_true_peak_os)
 * and the meter aggregates (as omega_meter_update) for n_frames x n_channels channel-frames of length
 * m (frame-major, contiguous), with one host round trip when mem = OMEGA_MEM_HOST (the three entry
 * points each stage, launch and synchronize on their own). lufs_inst / tp_db may be NULL (device
 * scratch), meters [n_cf, 5] is required. The true peak runs on the context's side stream beside the
 * weighting; for power-of-two frame lengths it counts in on a device counter that the aggregates
 * poll (bounded, OMEGA_EHIP on expiry), so the caller's stream joins the side stream by an event only
 * when other meter work went there since the last call. Outputs are bitwise those of the three calls. */
int omega_calculate_lufs(omega_ctx* ctx, const float* x, int64_t n_frames, int32_t m, int32_t mode,
                         int32_t oversampling, float* lufs_inst, float* tp_db, double* meters, int mem);

/* ---- band reductions (A10/A11) ---- */
typedef struct omega_bands omega_bands;
typedef enum { OMEGA_BANDS_MAX = 0, OMEGA_BANDS_MEAN = 1 } omega_band_op;
/* n_bands bands [starts[i], ends[i]) over spectra of n_bins bins. MAX: out[i] = max(spec[s:e]) *
 * scale[i] (pipeline.py:313-324); MEAN: out[i] = mean((spec*bin_scale)[s:e]) (freq_mapper.py:180-194).
 * scale / bin_scale may be NULL (ones). Bands whose end exceeds n_bins are 0 (MAX) or stop the
 * table (MEAN, freq_mapper.py:188-189), exactly as the reference. */
int omega_bands_create(omega_ctx* ctx, int op, const int32_t* starts, const int32_t* ends,
                       int32_t n_bands, int32_t n_out, const double* scale, const double* bin_scale,
                       int32_t n_bins, omega_bands** out);
void omega_bands_destroy(omega_bands* b);
int omega_bands_apply(omega_ctx* ctx, omega_bands* b, const float* spec, int64_t n, int64_t spec_stride,
                      float* out, int mem);

/* ---- chromagram (A12) over n spectra of n_bins bins with uniform rfftfreq spacing df ---- */
int omega_chroma(omega_ctx* ctx, const float* spec, int64_t n, int32_t n_bins, double df,
                 double* out_raw, int mem);

/* ---- windowed R2C FFT (A13): magnitude [n, m/2+1] and/or complex [n, m/2+1] (interleaved) ---- */
int omega_rfft(omega_ctx* ctx, const float* x, int64_t n, int32_t m, int32_t window, float* mag,
               float* cplx, int mem);

/* ---- fused spectrum analysis (BASELINE cfg3): per frame of m samples (m = 8192), the windowed
 * rfft magnitude (A13), the log-band max of a MAX band table (A10, before smoothing; bands may be
 * NULL) and the chromagram before its temporal blend (A12, bins at df = sample_rate / m), reading
 * each frame once. Any output may be NULL: bands_out [n, n_out], chroma_out [n, 12], mag_out
 * [n, m/2+1]. Replaces the BatchedFFTProcessor -> map_to_bands / compute_chromagram chain
 * (batched_fft_processor.py:148-285, pipeline.py:295-335, chromagram.py:109-159). ---- */
/* Drum-detection spectral features of consecutive magnitude frames of ONE stream (SURVEY.md §8(f)
 * row 1) -- replaces the per-frame feature part of omega4/analyzers/drum_detection.py
 * EnhancedKickDetector.detect_kick_onset :80-103 (calculate_band_flux :47-67,
 * calculate_adaptive_threshold :69-78) and EnhancedSnareDetector.detect_snare_onset :268-305
 * (calculate_multi_band_flux :231-266, calculate_spectral_centroid :212-229); the onset decisions read
 * the wall clock and stay with the caller. mag: n_frames rows of n_bins float32 magnitudes, row
 * stride mag_stride floats. out: [n_frames, 14] float64 = kick sub/body/click flux, kick sub/body/click
 * threshold, snare fundamental/body/snap/rattle flux, snare fundamental/body/snap threshold, snare
 * spectral centroid (Hz). The context keeps the stream state (previous frame, 21-deep flux histories)
 * across calls; omega_drum_reset starts a new stream. n_bins is fixed per context. */
int omega_drum_features(omega_ctx* ctx, const float* mag, int64_t n_frames, int32_t n_bins, int64_t mag_stride,
                        double sensitivity, double* out, int mem);
int omega_drum_reset(omega_ctx* ctx);

/* App spectrum post-processing of combined spectra -- replaces the per-frame
 * part of omega4_main.ProfessionalLiveAudioAnalyzer after combine_results_optimized:
 * process_multi_resolution_fft :748-752 (equal-loudness curve, bass boost), update_content_type
 * :805-840, process_audio_spectrum :991-1056 (98th-percentile normalisation,
 * apply_frequency_compensation :855-926, optional max normalisation, band means -> sqrt -> clamp,
 * frequency-dependent band EMA). omega_post_configure uploads the host-built tables (host memory):
 * curve[T] equal-loudness by position, bass[T] (combine frequency < 250 Hz), comp_instr / comp_vocal
 * [T] compensation factors, vocal_sup[T], ranges {bass_end, vocal_start, vocal_end, high_start},
 * the percentile's sorted ranks and float32 gamma, bands [n_bands] (start, end) already truncated
 * as the reference's loop does, band_smooth[n_bands] = the EMA factor f of each band (in [0, 1]).
 * omega_post_process (device memory only): n_frames spectra at row stride `stride` -> spectrum_out
 * [n, T] float32, bands_out [n, n_bands] float64 (after the EMA, which runs across frames in order and
 * across calls), content_out [n] (0 instrumental, 1 vocal, 2 bass-heavy; may be NULL). flags:
 * OMEGA_POST_*. Bands are numpy's values bit for bit: a frame's band list is float32, or float64 when
 * a band clamps to the Python int 1 (:1034: max(0, min(1, v)) returns the int), and the EMA
 * (:1041-1054) runs in the dtypes numpy gives each term -- bands_out holds both exactly. (A frame
 * whose every band clamps would make numpy's array int64; after the 98th-percentile normalisation
 * to 0.8 no frame reaches that.) */
enum {
  OMEGA_POST_PSYCHO = 1,      /* equal-loudness curve + bass boost */
  OMEGA_POST_FREQ_COMP = 2,   /* apply_frequency_compensation */
  OMEGA_POST_NORMALIZE = 4,   /* final max normalisation */
  OMEGA_POST_SMOOTH = 8       /* band EMA */
};
int omega_post_configure(omega_ctx* ctx, int32_t n_bins, const double* curve, const uint8_t* bass,
                         const float* comp_instr, const float* comp_vocal, const float* vocal_sup,
                         const int32_t* ranges, int32_t p_lo, int32_t p_hi, float p_gamma,
                         const int32_t* band_start, const int32_t* band_end, const double* band_smooth,
                         int32_t n_bands);
int omega_post_process(omega_ctx* ctx, const float* spectra, int64_t n_frames, int64_t stride, int32_t flags,
                       float bass_boost, float* spectrum_out, double* bands_out, int32_t* content_out);
int omega_post_reset(omega_ctx* ctx);
int omega_spectra(omega_ctx* ctx, const float* x, int64_t n, int32_t m, int32_t window, omega_bands* bands,
                  float* bands_out, double* chroma_out, float* mag_out, int mem);


/* VU meter ballistics, VUMetersPanel.update (omega4/panels/vu_meters.py:55-99), for n_updates
 * consecutive update(audio, dt) calls of every channel (one stream each; the reference duplicates its
 * mono input into L and R): update u of channel c reads chunk samples at x + u*update_stride +
 * c*channel_stride (float32, or float64 when f64 != 0 -- the app passes its float64 windowed frame);
 * dt[n_updates] in seconds. out [n_updates, C, 3] float64: the VU level (dBFS + 18 over the last
 * int(0.3 fs) samples, -60 + 18 when silent), the damped display value and the peak hold. The sample
 * history and the needle state carry over between calls; omega_vu_reset starts over. */
int omega_vu_update(omega_ctx* ctx, const void* x, int32_t f64, int64_t n_updates, int32_t chunk, int64_t update_stride,
                    int64_t channel_stride, const double* dt, double* out, int mem);
int omega_vu_reset(omega_ctx* ctx);

/* TransientAnalyzer.analyze_transients (omega4/analyzers/transient.py:19-108) for n_frames frames of
 * n samples (any n >= 64, as the reference; float32, or float64 when f64 != 0), frame f at x + f*frame_stride,
 * in float64 like scipy: Hilbert envelope, Savitzky-Golay (21, 3) smoothing, attack points where the
 * envelope's derivative exceeds twice its standard deviation. out [n_frames, 6] float64:
 * transients_detected, attack_time (ms), punch_factor, envelope_peak, envelope_rms and the smoothed
 * envelope's mean (the value the reference appends to its envelope_history). */
int omega_transients(omega_ctx* ctx, const void* x, int32_t f64, int64_t n_frames, int32_t n, int64_t frame_stride,
                     double* out, int mem);

/* CepstralAnalyzer.detect_pitch_advanced (omega4/panels/pitch_detection.py:485-556; ABI 4) for n_frames
 * frames of n samples (2048, 4096 or 8192; float32, or float64 when f64 != 0 -- cast to float32 on load
 * as :587-588 does), frame f at x + f*frame_stride (frame_stride may be smaller than n: an overlapping
 * stream). Three methods per frame and their confidence-weighted combination:
 *   cepstrum         float64: order-4 Butterworth high-pass (sosfilt, zero state) + RMS compression
 *                    (:497-525), Hann window, rfft, log(|X| + 1e-10), irfft (:132-144), the strongest
 *                    find_peaks peak of the period range (:146-174)
 *   autocorrelation  x - mean, zero-padded to 2n, irfft(|rfft|^2) / (r[0] + 1e-10) (:176-195), the first
 *                    peak find_peaks(height=0.3, distance=20) keeps (:197-227)
 *   YIN              the vectorised path over the first yin_window_size samples (:229-316, :363-371)
 *   combine          :373-433 with the acceptance thresholds 0.15 / 0.2 / 0.25 and the weights 0.8 / 0.9 /
 *                    1.1 the reference hard-codes (it does not read its config's *_weight fields)
 * omega_pitch_configure designs the high-pass sections (scipy.signal.butter's closed form; order 4, the
 * order of every reference preset -- other orders return OMEGA_EUNSUP) and stores the settings; it must
 * precede omega_pitch_detect. out [n_frames, 10] float64: pitch, confidence, cepstral pitch and
 * confidence, autocorrelation pitch and confidence, YIN pitch and confidence, the frame's RMS, flags
 * (bit 0: non-finite samples, bit 1: RMS below 1e-6 -- validate_audio_input :79-91). A flagged frame's
 * first eight columns are zero; it does not affect the other frames of the batch. n < yin_window_size
 * gives the reference's all-zero result (:487-495); any other n outside {2048, 4096, 8192} returns
 * OMEGA_EUNSUP. The note name, stability and histories (:435-483) are scalar host work left to the caller. */
typedef struct {
  int32_t sample_rate;
  double min_pitch, max_pitch;       /* Hz; periods int(fs / max_pitch) .. int(fs / min_pitch) */
  double yin_threshold;
  int32_t yin_window_size;           /* after PitchDetectionConfig.adjust_for_sample_rate */
  int32_t enable_preprocessing;
  double highpass_frequency;
  int32_t highpass_order;            /* 4 */
  int32_t enable_compression;
  double compression_threshold, compression_ratio;
} omega_pitch_config;
/* PitchDetectionConfig's defaults at 48 kHz (pitch_detection_config.py:13-121): 50..2000 Hz, window 1920. */
void omega_pitch_config_default(omega_pitch_config* cfg);
int omega_pitch_configure(omega_ctx* ctx, const omega_pitch_config* cfg);
int omega_pitch_detect(omega_ctx* ctx, const void* x, int32_t f64, int64_t n_frames, int32_t n, int64_t frame_stride,
                       double* out, int mem);

/* HarmonicAnalyzer.detect_harmonic_series (omega4/panels/harmonic_analysis.py:193-333; ABI 5) for
 * n_frames frames: the float32 spectrum of n_bins magnitudes at spectra + f*spec_stride over the float64
 * frequency table given to omega_harmonic_configure, and -- optionally -- the frame's m audio samples
 * (float32, or float64 when f64 != 0; widened to float64 on load) at audio + f*audio_stride for the LPC
 * formants. audio == NULL is the reference's audio_data=None: no formants.
 *   peaks      scipy.signal.find_peaks(height = 0.1 max, distance = 10) with scipy's plateau rule (the
 *              middle of a flat top) and its distance rule over all peaks, highest first
 *   series     per surviving peak with 20 <= f <= 2000 Hz up to 16 harmonics (:281-333); kept when the
 *              strength score exceeds 0.3, sorted by strength (descending, stable)
 *   metrics    for the first series' fundamental: THD, THD+N, centroid, spread, rolloff, flux against the
 *              previous frame, inharmonicity, HNR (harmonic_metrics.py:51-357); all 0 without a series
 *   formants   detect_formants_lpc (:115-196): order 14, the reference's recursion as written, the roots
 *              by a simultaneous iteration; only when a series was found
 * out [n_frames, 16] float64: series count (the true count, even above max_series), dominant
 * fundamental, thd, thd_plus_noise, centroid, spread, flux, rolloff, inharmonicity, hnr_db, formant
 * count, F1..F4, flags (bit 0: the root iteration did not converge -- no formants; bit 1: non-finite
 * input -- a non-finite spectrum gives the zero row). series_bins [n_frames, max_series, 17] int32: the
 * peak bin, then the bin of harmonic n = 1..16 or -1 where it was not accepted (rows past the count are
 * -1); series_strength [n_frames, max_series] float64 in the sorted order. Both may be NULL.
 * Flux state: frame f compares with frame f-1 of the call, frame 0 with the spectrum the context kept
 * from the previous call (flux 0 when there is none); the call's last spectrum is kept whether or not it
 * had a series (a non-finite spectrum too: the next frame's flux leaves its non-finite bins out and that
 * frame carries flag bit 1). omega_harmonic_reset forgets it; omega_harmonic_configure (which must precede
 * omega_harmonic_analyze and may be repeated with another table) does too.
 * Supported: 16 <= n_bins <= 8193, strictly increasing freqs, 15 <= m <= 8192; other sizes return
 * OMEGA_EUNSUP, a non-increasing table or max_series outside 1..1024 OMEGA_EINVAL. Instrument matching
 * (:335-431) and the vowel lookup are scalar host work left to the caller. */
typedef struct {
  int32_t sample_rate;
  int32_t n_bins;                    /* entries of freqs and bins per spectrum */
  int32_t max_series;                /* rows of series_bins / series_strength per frame */
} omega_harmonic_config;
/* 48000 Hz, 512 bins (the app's combined spectrum), 16 series. */
void omega_harmonic_config_default(omega_harmonic_config* cfg);
int omega_harmonic_configure(omega_ctx* ctx, const omega_harmonic_config* cfg, const double* freqs);
int omega_harmonic_analyze(omega_ctx* ctx, const float* spectra, int64_t spec_stride, const void* audio, int32_t f64,
                           int32_t m, int64_t audio_stride, int64_t n_frames, double* out, int32_t* series_bins,
                           double* series_strength, int mem);
int omega_harmonic_reset(omega_ctx* ctx);
/* The HarmonicMetrics methods for ONE frame and a fundamental the caller names (harmonic_metrics.py:51-357),
 * stateless like the reference's: the same kernels and the same `out` row as omega_harmonic_analyze, but
 * thd, thd_plus_noise, inharmonicity and hnr_db are evaluated for `fundamental` (all 0 when it is <= 0),
 * centroid / spread / rolloff and the formants (when audio != NULL) whether or not the spectrum holds a
 * harmonic series, and the flux against `previous` (n_bins values; NULL: 0). Columns 0 and 1 are the
 * series count found and `fundamental`. The stream state of omega_harmonic_analyze is neither read nor
 * written. */
int omega_harmonic_metrics(omega_ctx* ctx, const float* spectrum, const float* previous, const void* audio,
                           int32_t f64, int32_t m, double fundamental, double* out, int mem);

/* GenreClassifier.extract_features (omega4/panels/genre_classification.py:175-254 with the compute_* /
 * estimate_* helpers, :256-422 and :600-783) for n_frames frames of one stream: the float32 spectrum of
 * n_bins values at spectra + f*spec_stride (its magnitude is taken) over the float64 frequency table given
 * to omega_genre_configure, and the frame's m audio samples (float32, or float64 when f64 != 0) at
 * audio + f*audio_stride; rows may overlap. The entry points are additive to ABI 5: a caller detects them
 * by their presence.
 * out [n_frames, OMEGA_GENRE_COLS] float64, in this order:
 *    0 spectral_centroid        float64 sum / np.sum(magnitude) (float32 pairwise); 0 for a zero sum
 *    1 spectral_rolloff         freqs[min(index, n_bins - 1)]; 0 for a zero sum
 *    2 rolloff_index            first index of the SEQUENTIAL float32 np.cumsum >= float32(0.85) cumsum[-1]
 *    3 zero_crossings           count of nonzero np.diff(np.sign(x)) (the rate is this / m)
 *    4 spectral_bandwidth
 *    5 dynamic_range            min(1, (loud - quiet) / loud) if quiet > 0 else 0
 *    6 loud, 7 quiet            np.percentile(|x|, 95) and (|x|, 20), in the audio's precision
 *    8 rms                      np.sqrt(np.mean(x ** 2)) (the panel's silence gate; the device does not gate)
 *    9 spectral_complexity      1 - flatness over 100..4000 Hz, evaluated in float64; 0.3 where the reference says so
 *   10 bass_emphasis, 11 vocal_presence, 12 high_freq_energy   float32, operation for operation
 *   13 spectral_flux            against the previous frame's magnitude; 0 for the first frame after
 *                               configure / reset
 *   14 distortion_count         qualifying peaks among the five largest (harmonic_distortion = min(0.2 x, 1))
 *   15 mid_frequency_dominance
 *   16 flags                    bit 1: non-finite input. A frame with a non-finite sample or bin gives the
 *                               zero row; its magnitude is stored like any other, the next frame's flux
 *                               leaves the non-finite bins out and carries the flag
 * peak_bins [n_frames, OMEGA_GENRE_PEAKS] int32: the bins of the five largest strict local maxima above
 * float32(np.mean(magnitude) * 2), largest first, ties to the lower bin, -1 past their number.
 * Flux state: frame f compares with frame f-1 of the call, frame 0 with the magnitude the context kept
 * from the previous call; omega_genre_reset forgets it, omega_genre_configure (which must precede
 * omega_genre_features and may be repeated with another table) does too. It is a state of its own, apart
 * from omega_harmonic_analyze's.
 * Supported: 16 <= n_bins <= 8193, strictly increasing freqs, 15 <= m <= 8192; other sizes return
 * OMEGA_EUNSUP. The drum, harmonic-series, chroma and history features and classify() are scalar host work
 * left to the caller. */
#define OMEGA_GENRE_COLS 17
#define OMEGA_GENRE_PEAKS 5
typedef struct {
  int32_t sample_rate;
  int32_t n_bins;                    /* entries of freqs and bins per spectrum */
} omega_genre_config;
/* 48000 Hz, 512 bins (the app's combined spectrum). */
void omega_genre_config_default(omega_genre_config* cfg);
int omega_genre_configure(omega_ctx* ctx, const omega_genre_config* cfg, const double* freqs);
int omega_genre_features(omega_ctx* ctx, const float* spectra, int64_t spec_stride, const void* audio, int32_t f64,
                         int32_t m, int64_t audio_stride, int64_t n_frames, double* out, int32_t* peak_bins, int mem);
int omega_genre_reset(omega_ctx* ctx);

/* HipHopDetector.analyze (omega4/panels/hip_hop_detector.py:94-154 with the helpers it calls, :156-384) for
 * n_frames independent frames: the float32 spectrum of n_bins values at spectra + f*spec_stride (its magnitude
 * is taken) over the float64 frequency table given to omega_hiphop_configure, and the frame's m audio samples
 * (float32, or float64 when f64 != 0: rms and energies then follow numpy's float64) at audio + f*audio_stride;
 * rows may overlap. The reference filters every frame from the zero state, so the device keeps no state. The
 * entry points are additive to ABI 5: a caller detects them by their presence.
 * out [n_frames, OMEGA_HIPHOP_COLS] float64, in this order:
 *    0 rms                      np.sqrt(np.mean(x ** 2)) in the audio's precision (float32: bit for bit)
 *    1 sub_bass_presence        min(3 (0.3 t + 0.5 f + 0.2 min(s, 1)), 1): t the filtered RMS over rms (float64),
 *                               f and s the float32 power ratios
 *    2 kick_peak_count          find_peaks(|hilbert(kick band)|, height = mean + 1.5 std, distance = int(0.1 fs))
 *    3 kick_pattern_factor      what multiplies the caller's kick magnitude: 0.6 regularity + 0.4 (1 - syncopation)
 *                               of the peak spacings, 0.5 with at most one peak
 *    4 hihat_zero_crossings     count of nonzero np.diff(np.sign(hi-hat band)) (the rate is this / m)
 *    5 hihat_density            min(10 rate, 1) min(5 filtered RMS / rms, 1)
 *    6 spectral_tilt            float32, operation for operation
 *    7 vocal_peak_count         find_peaks(|spectrum[200..3000 Hz]|, prominence = float32(max * 0.3), distance = 20)
 *    8 vocal_presence           float32, operation for operation
 *    9 flags                    bit 0: silent (rms < 0.001, the reference's gate): every column but rms and
 *                               flags is 0. bit 1: non-finite input (a sample or a bin): the whole row is 0;
 *                               the other frames of the batch are unaffected
 *   10 sub_bass_rms, 11 hihat_rms   np.sqrt(np.mean(.)) of the two filtered signals (float64)
 *   12 envelope_threshold       mean + 1.5 np.std of the kick envelope
 *   13 sub_bass_power [20, 60], 14 bass_power [60, 250], 15 total_power (freqs < fs / 2: the Nyquist bin is left
 *      out), 16 low_energy [20, 500], 17 mid_energy [500, 2000], 18 high_energy [2000, 8000], 19 vocal_energy
 *      [200, 3000], 20 core_vocal_energy [300, 2000], 21 total_energy (every bin): np.sum(np.abs(.) ** 2) over
 *      the inclusive masks as numpy's float32 pairwise sums, bit for bit; 0 over a range without bins
 *   22 tilt_branch              0: no tilt (an empty band or zero energy), 1: plain, 2: boosted (low_ratio > 0.5),
 *                               3: boosted and clipped to 1
 *   23 vocal_branch             0: no value (no vocal bins, zero energy, or <= 10 vocal bins), 1: float32 value,
 *                               2: clipped to 1
 * kick_peaks [n_frames, OMEGA_HIPHOP_PEAKS] int32 (may be NULL): the kept envelope peaks in index order, -1 past
 * their number. The float64 columns that pass through the filters (1, 3, 5, 10-12) agree with scipy's sequential
 * sosfilt to 1e-9 relative (a 256-chunk float64 scan); the integer columns and the float32-path columns are exact.
 * kick_detected, the kick magnitude, the tempo stub, the confidence weights, the sub-genre and the 30-deep
 * histories are scalar host work left to the caller (omega_gpu.HipHopDetector restates them).
 * omega_hiphop_configure designs the three band-pass cascades (scipy.signal.butter(4, [lo, hi], 'bandpass',
 * fs=fs, output='sos'): sub-bass 20-60 Hz, kick 40-100 Hz, hi-hat 3000-min(10000, 0.9 fs/2) Hz) and stores the
 * masks' bin ranges; it must precede omega_hiphop_features and may be repeated with another table or rate.
 * omega_hiphop_get_sos returns the configured sections of filter `which` (0 sub-bass, 1 kick, 2 hi-hat) as
 * out[4][6] = b0 b1 b2 a0 a1 a2; omega_hiphop_design_sos designs them for a rate without a context.
 * Supported: sample_rate >= 8000 Hz (OMEGA_HIPHOP_PEAKS covers the floor((8192 - 3) / 800) + 1 = 11 peaks that
 * fit at that rate), 16 <= n_bins <= 8193, strictly increasing freqs, m a power of two 64..8192; other sizes
 * return OMEGA_EUNSUP. */
#define OMEGA_HIPHOP_COLS 24
#define OMEGA_HIPHOP_PEAKS 16
typedef struct {
  int32_t sample_rate;
  int32_t n_bins;                    /* entries of freqs and bins per spectrum */
} omega_hiphop_config;
/* 48000 Hz, 512 bins (the app's combined spectrum). */
void omega_hiphop_config_default(omega_hiphop_config* cfg);
int omega_hiphop_configure(omega_ctx* ctx, const omega_hiphop_config* cfg, const double* freqs);
int omega_hiphop_get_sos(omega_ctx* ctx, int32_t which, double* out);
int omega_hiphop_design_sos(int32_t sample_rate, int32_t which, double* out);
int omega_hiphop_features(omega_ctx* ctx, const float* spectra, int64_t spec_stride, const void* audio, int32_t f64,
                          int32_t m, int64_t audio_stride, int64_t n_frames, double* out, int32_t* kick_peaks,
                          int mem);

/* PhaseCorrelationPanel's analysis (omega4/panels/phase_correlation.py:124-220: _calculate_correlation, the
 * balance lines, _update_goniometer_enhanced, _calculate_band_correlations) for n_frames independent stereo
 * frames of m samples: frame f is at left + f*frame_stride and right + f*frame_stride, in elements (float32, or
 * float64 when f64 != 0; float32 is widened on load and everything downstream is float64). The planar
 * [F, 2, m] batch is right = left + m, frame_stride = 2m; rows may overlap. The reference's update() fabricates
 * its right channel from a mono frame with np.random; here both channels are the caller's. The device keeps no
 * state. The entry points are additive to ABI 5: a caller detects them by their presence.
 * out [n_frames, OMEGA_PHASE_COLS] float64, in this order:
 *    0 correlation      clip(mean(ln rn) / (std_l std_r), -1, 1) of the mean-centred channels (two passes: the
 *                       means, then the centred sums); 0.0 when a std is 0
 *    1 stereo_width     1 - |correlation|
 *    2 balance          (rms_right - rms_left) / (rms_right + rms_left); 0 when the sum is 0 (flag bit 1)
 *    3 rms_left, 4 rms_right   sqrt(mean(x^2))
 *    5 flags            bit 0: a non-finite sample in either channel: the whole row and the frame's points are
 *                       0; the other frames of the batch are unaffected. bit 1: rms_left + rms_right == 0 (the
 *                       reference leaves its balance untouched). bit 2: a time-domain std was 0 (the
 *                       reference's 0.0 fallback)
 *    6 band mask        bit b set: band b has at least one bin (the reference leaves the others untouched)
 *    7..16 band correlations   the same clipped correlation of |rfft(l np.hanning(m))| and |rfft(r np.hanning(m))|
 *                       over the bins with edges[b] <= f_k < edges[b + 1]; 0.0 for a band of one bin (its centred
 *                       values are 0) and for a band without bins
 * points [n_frames, OMEGA_PHASE_POINTS, 2] float64 (may be NULL): the goniometer's (x, y) of the samples
 * 0, step, 2 step, ... < m with step = max(1, m / 100), in the reference's operation order (bit for bit); 0 past
 * their number ceil(m / step).
 * Columns 0-2 and 7-16 agree with the reference called on float64 arrays to 1e-9 absolute, the RMS columns to
 * 1e-9 relative, on frames whose stds keep the margins tests/golden/gen_phase.py asserts (one m-point float64
 * transform of l w + i r w and lane-strided sums stand for numpy's two rffts and pairwise sums; the shared
 * transform leaves about 1e-16 of the louder channel's magnitudes in the other's bins, so an exactly silent
 * channel is given its exact zero spectrum and a channel some 200 dB below the other is not resolved).
 * omega_phase_band_ranges (no context, no device) turns the masks over np.fft.rfftfreq(m, 1 / sample_rate), in
 * numpy's own arithmetic (val = 1.0 / (m * (1.0 / fs)), f_k = k * val), into ranges[10][2] = [first, last);
 * first == last: no bins. edges are the caller's 11 band edges (the reference's np.logspace(log10(20),
 * log10(min(20000, fs / 2)), 11)); they are not recomputed here, because at 16000 Hz one ulp of the top edge
 * decides whether the Nyquist bin belongs to band 9. omega_phase_hanning writes np.hanning(m) as the library
 * computes and uploads it (numpy's route 0.5 + 0.5 cos(pi k / (m - 1)), k = 1 - m, 3 - m, ...), m >= 2.
 * omega_phase_configure stores the ranges and uploads the tables; it must precede omega_phase_correlation and
 * may be repeated. Supported: m a power of two 64..8192 (16 bytes of LDS per sample); other sizes return
 * OMEGA_EUNSUP. */
#define OMEGA_PHASE_BANDS 10
#define OMEGA_PHASE_COLS 17
#define OMEGA_PHASE_POINTS 128 /* max over supported m of ceil(m / max(1, m / 100)) */
typedef struct {
  int32_t sample_rate;
  int32_t m;                         /* samples per frame and channel */
} omega_phase_config;
/* 48000 Hz, 2048 samples. */
void omega_phase_config_default(omega_phase_config* cfg);
int omega_phase_band_ranges(int32_t sample_rate, int32_t m, const double* edges, int32_t* ranges);
int omega_phase_hanning(int32_t m, double* out);
int omega_phase_configure(omega_ctx* ctx, const omega_phase_config* cfg, const double* edges);
int omega_phase_correlation(omega_ctx* ctx, const void* left, const void* right, int32_t f64, int64_t frame_stride,
                            int64_t n_frames, double* out, double* points, int mem);

/* RoomModeAnalyzer (omega4/analyzers/room_modes.py:71-239 detect_room_modes with estimate_q_factor and
 * classify_room_mode; :356-458 the Schroeder and EDT decay estimates), all in float64 (float32 input is widened
 * on load). The device keeps no state. The entry points are additive to ABI 5.
 * omega_room_bin_range (no context, no device) applies the mask (freqs >= min_f) & (freqs <= max_f) to the
 * caller's table (the app passes np.linspace(0, fs / 2, n), not rfftfreq; it is never recomputed here) and writes
 * range[2] = [first, last); OMEGA_EINVAL unless freqs is strictly increasing.
 * omega_room_configure stores the range and the thresholds and uploads the table; it must precede the two calls
 * below and may be repeated. hints (may be NULL): the six frequencies classify_room_mode derives from the room
 * dimension hints -- the axial fundamentals speed / (2 length), speed / (2 width), speed / (2 height), then the
 * three tangential frequencies in the reference's order; NULL or any entry <= 0: no hints. More than
 * OMEGA_ROOM_MAX_BINS bins in range return OMEGA_EUNSUP.
 * omega_room_modes: n_frames spectra of n_bins values, frame f at spectra + f*spec_stride elements (rows may
 * overlap). out [n_frames, OMEGA_ROOM_ROWS, OMEGA_ROOM_COLS] float64: row 0 is the header
 *    0 count   the full number of modes          1 flags   bit 0: a non-finite bin in the whole spectrum or the
 *    2 mean    np.mean of the in-range bins                table (no modes; other frames are unaffected);
 *    3 std     np.std of them (two passes)                 bit 1: mean or std is 0, or no bin in range (no
 *                                                          modes); bit 2: more than OMEGA_ROOM_MAX_MODES modes
 * and rows 1.. are the first OMEGA_ROOM_MAX_MODES modes by severity descending, ties by ascending bin (Python's
 * stable sorted(reverse=True)), zero past the count:
 *    0 frequency  1 magnitude  2 q_factor  3 severity  4 type  5 prominence  6 bandwidth  7 bin (in the table)
 * type = base + 8 harmonic; base 0 axial_length, 1 axial_width, 2 axial_height, 3 tangential, 4 oblique; harmonic
 * 1..3 for the "_H<n>" types of a hinted room, else 0. The peak set is scipy's find_peaks(x, height = mean *
 * peak_threshold_multiplier, prominence = std * minimum_prominence_std). frequency, magnitude, prominence,
 * q_factor and bandwidth are the reference's IEEE operations on exact inputs, bit for bit; mean, std and
 * severity agree to 1e-12 relative on frames with std >= 1e-3 mean (block sums stand for numpy's pairwise
 * sums), and the peak set is the reference's where no height, prominence or severity decision lies within
 * 1e-9 relative of its threshold.
 * omega_room_decay: n_streams histories of L samples (2 <= L <= 2^20; longer: OMEGA_EUNSUP), stream s at
 * audio + s*stream_stride elements. out [n_streams, OMEGA_ROOM_RT60_COLS] float64:
 *    0 curve[0]   the sum of squares (before the 1e-10 floor)
 *    1 idx5, 2 idx10, 3 idx35   the first index with 10 log10(curve / curve[0]) <= -5, -10, -35; L: none
 *    4 slope, 5 intercept   of the least-squares line of the dB curve on i / sample_rate over [idx5, idx35)
 *    6 r_squared  1 - SSR / SST of that line
 *    7 flags      bit 0: a non-finite sample or square (the other columns are 0); bit 1: idx5 or idx35 is
 *                 missing or idx35 <= idx5; bit 2: fewer than 3 points in [idx5, idx35); bit 3: slope >= 0.
 *                 With bit 1 or 2 set columns 4-6 are 0.
 * W > 0 (it must divide L) and energies [n_streams, L / W] non-NULL: also the sum of squares of every frame of
 * W samples. slope, intercept and curve[0] agree with the reference called on float64 arrays to 1e-9 relative,
 * r_squared to 1e-9 absolute, the indices exactly where the dB curve keeps 1e-9 dB from the thresholds. */
#define OMEGA_ROOM_MAX_MODES 64
#define OMEGA_ROOM_ROWS 65
#define OMEGA_ROOM_COLS 8
#define OMEGA_ROOM_MAX_BINS 4096
#define OMEGA_ROOM_RT60_COLS 8
typedef struct {
  double sample_rate;
  double min_frequency, max_frequency;
  double peak_threshold_multiplier, minimum_prominence_std;
  double min_q_factor, max_q_factor;
  double minimum_severity;
} omega_room_config;
/* 48000 Hz and RoomModeConfig's defaults: 30..300 Hz, 2.0, 1.0, Q 0.5..100, severity 0.3. */
void omega_room_config_default(omega_room_config* cfg);
int omega_room_bin_range(const double* freqs, int32_t n_bins, double min_f, double max_f, int32_t* range);
int omega_room_configure(omega_ctx* ctx, const omega_room_config* cfg, const double* freqs, int32_t n_bins,
                         const double* hints);
int omega_room_modes(omega_ctx* ctx, const void* spectra, int32_t f64, int64_t spec_stride, int64_t n_frames,
                     double* out, int mem);
int omega_room_decay(omega_ctx* ctx, const void* audio, int32_t f64, int64_t stream_stride, int64_t L, int64_t W,
                    int64_t n_streams, double* out, double* energies, int mem);

/* VoiceDetectionPanel (omega4/panels/voice_detection.py:57-122 detect_voice with _detect_formant_structure,
 * :169-192 the autocorrelation of detect_pitch) for a batch of independent frames; the device keeps no state.
 * The entry points are additive to ABI 5.
 * omega_voice_bin_range (no context, no device): range[2] = [voice_start, voice_end] =
 * np.searchsorted(freq_bins, 85), np.searchsorted(freq_bins, 255) over freq_bins = np.fft.rfftfreq(frame_len,
 * 1 / sample_rate) as numpy evaluates it, arange * (1.0 / (frame_len * (1 / sample_rate))).
 * omega_voice_configure fixes the shape and may be repeated. Built: n_bins 1..OMEGA_VOICE_MAX_BINS, frame_len a
 * power of two 64..8192, sample_rate >= 8000; anything else returns OMEGA_EUNSUP and leaves the configured shape
 * as it was.
 * omega_voice_features: frame f has its spectrum (n_bins float32) at spectra + f*spec_stride and its m = frame_len
 * samples (float32, or float64 when f64) at frames + f*frame_stride, both in elements; rows may overlap. The
 * samples are read only where a pitch can be taken at all (frame_len >= 2048 and int(sample_rate / 80) <
 * frame_len); otherwise frames may be NULL. out [n_frames, OMEGA_VOICE_COLS] float64:
 *    0 flags         bit 0: the range check voice_start < n_bins and voice_end < n_bins failed (the reference
 *                    leaves its state as it was); bit 1: total_energy <= 0; bit 2: a non-finite bin or sample
 *                    (every other column is 0; other frames are unaffected); bit 3: no pitch for this shape
 *    1 voice_start, 2 voice_end
 *    3 voice_energy  sum(spectrum[voice_start:voice_end]), 4 total_energy  sum(spectrum): float64 sums of the
 *                    float32 bins (0 with bit 0)
 *    5 formant_count the ranges 200-900, 800-2500, 2000-3500, 3000-4500 Hz (ends included) that hold a peak
 *    6..9 the bin and 10..13 freq_bins[bin] of each range's first peak, 0 where the range holds none (a peak is
 *                    never bin 0). One peak may serve two ranges. All 0 with bit 0 or 1, or n_bins <= 10.
 *    14 corr0        c[0] of c[l] = sum_n x[n] x[n + l] in float64
 *    15 peak_lag     np.argmax over l in [int(sample_rate / 400), int(sample_rate / 80)), the first of equal maxima
 *    16 corr_peak    c[peak_lag]; 14..16 are 0 with bit 3
 * The peaks are those of scipy.signal.find_peaks(smoothed, prominence=np.max(smoothed) * 0.1) with smoothed =
 * scipy.signal.savgol_filter(spectrum, min(11, n_bins // 4 * 2 + 1), 3) in float32; smoothed is within 1 ulp of
 * scipy's, so the peak set is the reference's where no comparison of neighbouring smoothed values and no
 * prominence lies that close to its decision. Frequencies are bit-equal to numpy's; the sums agree with a
 * float64 evaluation to 1e-12 relative, corr0 and corr_peak to 1e-9 of corr0. */
#define OMEGA_VOICE_COLS 17
#define OMEGA_VOICE_MAX_BINS 8193
typedef struct {
  double sample_rate;
  int32_t n_bins;     /* bins per spectrum (the app: 1025) */
  int32_t frame_len;  /* samples per audio frame (the app: 2048) */
} omega_voice_config;
/* 48000 Hz, 1025 bins, 2048 samples. */
void omega_voice_config_default(omega_voice_config* cfg);
int omega_voice_bin_range(double sample_rate, int32_t frame_len, int32_t* range);
int omega_voice_configure(omega_ctx* ctx, const omega_voice_config* cfg);
int omega_voice_features(omega_ctx* ctx, const float* spectra, int64_t spec_stride, const void* frames, int32_t f64,
                         int32_t m, int64_t frame_stride, int64_t n_frames, double* out, int mem);

/* TransientDetectionPanel (omega4/panels/transient_detection.py:79-365) for consecutive frames of one stream: every
 * frame-local quantity of update(), and the two that compare a frame with the ones before it (spectral flux,
 * phase-deviation novelty). The context keeps nothing between calls: the caller carries the stream's state, a blob
 * of omega_tdetect_state_size() float64 values (the last flux spectrum, the last two phase rows, validity flags),
 * from state_out of one call to state_in of the next. state_in NULL: a stream's first frames. state_out NULL: not
 * wanted. Both live where `mem` says and may be the same buffer. One call on F frames equals F one-frame calls
 * chained through the blob, bit for bit. The entry points are additive to ABI 5.
 * omega_tdetect_configure fixes the shape and may be repeated. Built: frame_len a power of two 256..8192, n_bins
 * 2..OMEGA_TDETECT_MAX_BINS, sample_rate >= 8000; anything else returns OMEGA_EUNSUP and leaves the configured
 * shape as it was.
 * omega_tdetect_band_indices (no context, no device): idx[5] = np.searchsorted(freqs, [0, 100, 250, 2000, fs / 2])
 * over freqs = np.fft.rfftfreq(2 (n_bins - 1), 1 / sample_rate) as numpy evaluates it.
 * omega_tdetect_features: frame f has its spectrum (n_bins float32 magnitudes) at spectra + f*spec_stride and its
 * frame_len samples (float32, widened exactly, or float64 when f64) at frames + f*frame_stride, both in elements;
 * rows may overlap. All arithmetic is float64. out [n_frames, OMEGA_TDETECT_COLS] float64:
 *    0 flags        bit 0: a non-finite sample or bin (every other column is 0, and the frame is passed over as a
 *                   predecessor: the state goes on as if it had not come); bit 1: no HF column for this shape
 *                   (frame_len 256, or 5000 Hz not below Nyquist); bit 2: no novelty for this shape (frame_len <
 *                   1024); bit 3: no frame before this one, flux is 0; bit 4: no frame before this one, novelty is 0
 *    1 envelope     mean(savgol_filter(abs(hilbert(x)), 11, 3))
 *    2 peak         max |x|            3 energy       sum x^2
 *    4 flux_sum     sum(S), S = abs(rfft(x[:512] * hanning(512)))[:128] (zero-padded at frame_len 256)
 *    5 flux         sum(max(0, S - S_prev))
 *    6 novelty      sum(mag * min(|phase - (2 phase_1 - phase_2)|, pi)) over the 513 bins of rfft(pre[-1024:] *
 *                   hanning(1024)), pre[n] = x[n] - 0.97 x[n-1] with pre[0] = x[0]; a stream's second frame takes
 *                   phase_2 = phase_1 as the reference seeds them; no phase is wrapped
 *    7 mag_sum      sum(mag) of those bins (0 with bit 2)
 *    8 hf_energy    sum(filtfilt(*butter(4, 5000 / (fs / 2), 'high'), x) ** 2) (0 with bit 1)
 *    9 sign_diff    sum |diff(sign x)| (an integer; the zero-crossing rate is this over 2 frame_len)
 *   10 peak_idx     the first argmax |x|
 *   11 start_idx    the nearest i < peak_idx with |x_i| < 0.1 peak, else 0
 *   12 end_idx      the nearest i > peak_idx with |x_i| < 0.1 peak, else frame_len - 1
 *   13 spec_sum     sum(s)            14 spec_fsum   sum(freqs * s)
 *   15 rolloff_idx  the first i whose float64 prefix sum reaches 0.85 spec_sum (0 where spec_sum <= 0)
 *   16..19 band sums s[idx[b]:idx[b+1]], 0 where the band's guard bit is clear
 *   20 guards       bit b: idx[b] < n_bins and idx[b+1] < n_bins (the reference keeps a band's old value otherwise)
 * Sums of the spectrum agree with a float64 evaluation to 1e-12 relative; the transform- and filter-derived
 * columns to 1e-9 (hf_energy relative to energy, novelty relative to pi mag_sum). */
#define OMEGA_TDETECT_COLS 21
#define OMEGA_TDETECT_MAX_BINS 8193
typedef struct {
  double sample_rate;
  int32_t n_bins;     /* bins per spectrum (the app: 513) */
  int32_t frame_len;  /* samples per audio frame (the app: 2048) */
} omega_tdetect_config;
/* 48000 Hz, 513 bins, 2048 samples. */
void omega_tdetect_config_default(omega_tdetect_config* cfg);
int omega_tdetect_band_indices(double sample_rate, int32_t n_bins, int32_t* idx);
int omega_tdetect_configure(omega_ctx* ctx, const omega_tdetect_config* cfg);
int64_t omega_tdetect_state_size(void);
int omega_tdetect_features(omega_ctx* ctx, const float* spectra, int64_t spec_stride, const void* frames, int32_t f64,
                           int64_t n_frames, int64_t frame_stride, const double* state_in, double* state_out,
                           double* out, int mem);

/* BassZoomPanel (omega4/panels/bass_zoom.py:51-97, :141-232) for consecutive frames of one stream: the 20..200 Hz
 * bars of a Hann-windowed 8192-point spectrum, their smoothing and their peak hold. The context keeps nothing
 * between calls: the caller carries the panel's state, a blob of omega_basszoom_state_size() float64 values (64
 * bar values, 64 peak values, 64 peak timestamps; the first n_bars of each are used, the float32 state widened
 * exactly), from state_out of one call to state_in of the next. state_in NULL: a new panel (all zero). state_out
 * NULL: not wanted. Both live where `mem` says and may be the same buffer. One call on F frames equals F one-frame
 * calls chained through the blob, bit for bit. The entry points are additive to ABI 5.
 * omega_basszoom_mapping (no context, no device) reproduces setup_bass_mapping: the bins k of np.fft.rfftfreq(8192,
 * 1 / sample_rate), as numpy evaluates it, with 20 <= f <= 200 are first_bin .. first_bin + n_valid - 1; bar i holds
 * bins_per_bar = max(1, n_valid / 31) of them (the last bar may hold fewer); freq_ranges[2 i], [2 i + 1] are its
 * first and last bin's frequencies (the start not below the bar before's end) and compensation[i] is 0.3 / 0.6 /
 * 1.0 / 0.8 for a centre below 60 / 100 / 150 Hz / else. freq_ranges (2 OMEGA_BASSZOOM_MAX_BARS values) and
 * compensation (OMEGA_BASSZOOM_MAX_BARS values) may be NULL, as may every other output. OMEGA_EINVAL: a rate that is
 * not positive and finite. OMEGA_EUNSUP: no valid bin (a rate above 1638400 Hz; the reference then shows one bar
 * that never moves), more than OMEGA_BASSZOOM_MAX_BINS valid bins (rates below about 5760 Hz), or more than
 * OMEGA_BASSZOOM_MAX_BARS bars (no rate within the bin cap gives more than 61).
 * omega_basszoom_configure fixes the shape and may be repeated. Built: frame_len >= 1 (the first min(frame_len,
 * 8192) samples are read) at every rate the mapping accepts; frame_len 0 and every other rate return OMEGA_EUNSUP
 * and leave the configured shape as it was.
 * omega_basszoom_features: frame f has its samples (float32, widened exactly, or float64 when f64) at frames +
 * f*frame_stride, in elements; rows may overlap. times[f] is frame f's time in seconds (the reference reads
 * time.time() once per processed frame). All spectrum arithmetic is float64. Outputs, all float64:
 *   rows [n_frames, 3 + n_bars]   0 flags: bit 0, a non-finite sample (every other column is 0 and the frame is
 *                                 passed over: the state goes on as if it had not come)
 *                                 1 bass_max: the largest compensated bar mean of abs(rfft(x[:n] * hanning(n), 8192)),
 *                                 n = min(frame_len, 8192)
 *                                 2 scale_factor: 0.85 / bass_max * (log10(max(1, 10 bass_max)) / 2), 1 at bass_max 0
 *                                 3.. the bars scaled by it, those above 0.7 compressed to 0.7 + 0.3 (v - 0.7)
 *   bars, peaks, peak_times [n_frames, n_bars]   bar_values, peak_values (float32 values) and peak_timestamps
 *                                 after frame f: a rising bar takes 0.1 bar + 0.9 c, a falling one 0.6 bar + 0.4 c,
 *                                 clamped to [0, 1], in numpy 2.x's types (float32 products bar * float32(0.1),
 *                                 float64 products c * 0.9, their float64 sum rounded to float32); a bar above its
 *                                 peak sets the peak and its timestamp, else the peak takes the float32 product
 *                                 peak * float32(0.95) once times[f] - timestamp > 3.0
 * bass_max, scale_factor and the compressed values agree with a float64 evaluation to 1e-9 of the row's largest. */
#define OMEGA_BASSZOOM_MAX_BARS 64
#define OMEGA_BASSZOOM_MAX_BINS 256
typedef struct {
  double sample_rate;
  int32_t frame_len;  /* samples per audio frame (the app: 8192 and more) */
} omega_basszoom_config;
/* 48000 Hz, 8192 samples. */
void omega_basszoom_config_default(omega_basszoom_config* cfg);
int omega_basszoom_mapping(double sample_rate, int32_t* n_bars, int32_t* first_bin, int32_t* bins_per_bar,
                           int32_t* n_valid, double* freq_ranges, double* compensation);
int omega_basszoom_configure(omega_ctx* ctx, const omega_basszoom_config* cfg);
int64_t omega_basszoom_state_size(void);
int omega_basszoom_features(omega_ctx* ctx, const void* frames, int64_t frame_stride, int32_t f64, const double* times,
                            int64_t n_frames, const double* state_in, double* rows, double* bars, double* peaks,
                            double* peak_times, double* state_out, int mem);

/* BeatDetector / BeatDetectionPanel (omega4/panels/beat_detection.py:15-295, :297-384) and FrequencyBandTracker
 * (omega4/panels/frequency_band_tracker.py:26-240) for consecutive frames of one stream: the sums both panels take
 * over a frame's spectrum -- the spectral flux against the frame before, the kick band, the seven band energies,
 * the total, the centroid's numerator and the spread's -- and the beat panel's silence gate. The context keeps
 * nothing between calls: the caller carries the stream's state, a blob of omega_rhythm_state_size(n_bins) float64
 * values (a validity flag, n_bins, the last live frame's spectrum as exact float32 values), from state_out of one
 * call to state_in of the next. state_in NULL: a stream's first frames (a blob recorded for another n_bins counts
 * as none). state_out NULL: not wanted. Both live where `mem` says and may be the same buffer. One call on F frames
 * equals F one-frame calls chained through the blob, bit for bit. The entry points are additive to ABI 5.
 * omega_rhythm_configure fixes the shape and may be repeated; it needs no device until its arguments have passed.
 * freqs: the caller's frequency table, n_bins float64 values, uploaded when it differs from the configured one.
 * edges: OMEGA_RHYTHM_EDGES bin indices, np.argmax(freqs >= f) for f = 20, 50, 60, 120, 250, 500, 2000, 4000, 8000,
 * 20000 Hz, each 0..n_bins (else OMEGA_EINVAL). Where a band's UPPER edge is 0 the band runs to n_bins, the
 * reference's "beyond spectrum" rule (beat_detection.py:88-89, :146-147, frequency_band_tracker.py:121-122); a
 * lower edge is taken as it is. Built: n_bins 2..OMEGA_RHYTHM_MAX_BINS, frame_len 1..OMEGA_RHYTHM_MAX_FRAME;
 * anything else returns OMEGA_EUNSUP and leaves the configured shape as it was.
 * omega_rhythm_features: frame f has its spectrum (n_bins float32 values s) at spectra + f*spec_stride and, where
 * frames is not NULL, its frame_len samples x (float32, widened exactly, or float64 when f64) at frames +
 * f*frame_stride, both in elements; rows may overlap. frames NULL (the tracker's call): no gate, column 1 is 0.
 * All accumulation is float64. out [n_frames, OMEGA_RHYTHM_COLS] float64:
 *    0 flags        bit 0: a non-finite sample or bin (every other column is 0, and the frame is passed over: the
 *                   state goes on as if it had not come); bit 1: gated, sqrt(mean(x^2)) < 0.001 (:338-349) -- the
 *                   columns are there, but the frame is passed over as a predecessor, as the reference leaves
 *                   prev_spectrum untouched; bit 2: no live frame before this one in the stream, flux is 0
 *    1 sumsq        sum x^2
 *    2 spec_sum     sum s
 *    3 flux         sum max(0, float32(s - p)), p the predecessor's spectrum: the nearest earlier frame with
 *                   neither bit 0 nor bit 1, which may be the state's; the difference is rounded to float32 first
 *    4 kick         sum s[e50:e120]
 *    5..11 band0..6 sum s[lo:hi] for (20,60), (60,250), (250,500), (500,2000), (2000,4000), (4000,8000),
 *                   (8000,20000) Hz; 0 where lo >= hi
 *   12 spec_fsum    sum freqs s
 *   13 spread_sum   sum (freqs - c)^2 s with c = spec_fsum / (double)(float)spec_sum; 0 where spec_sum <= 0 or c <= 0
 * state_out: the last live frame of state_in followed by this call's frames; without one, state_in passes through.
 * Columns 1..12 agree with a float64 evaluation to 1e-12 relative, column 13 to 1e-9. */
#define OMEGA_RHYTHM_COLS 14
#define OMEGA_RHYTHM_EDGES 10
#define OMEGA_RHYTHM_MAX_BINS 8193
#define OMEGA_RHYTHM_MAX_FRAME 16384
typedef struct {
  int32_t n_bins;     /* bins per spectrum (the app: 513) */
  int32_t frame_len;  /* samples per audio frame (the app: 2048) */
} omega_rhythm_config;
/* 513 bins, 2048 samples. */
void omega_rhythm_config_default(omega_rhythm_config* cfg);
int omega_rhythm_configure(omega_ctx* ctx, const omega_rhythm_config* cfg, const double* freqs, const int32_t* edges);
/* 2 + n_bins (0 for n_bins < 1); no context, no device. */
int64_t omega_rhythm_state_size(int32_t n_bins);
int omega_rhythm_features(omega_ctx* ctx, const float* spectra, int64_t spec_stride, const void* frames, int32_t f64,
                          int64_t n_frames, int64_t frame_stride, const double* state_in, double* state_out,
                          double* out, int mem);

/* SpectrogramWaterfall / SpectrogramWaterfallPanel (omega4/panels/spectrogram_waterfall.py:56-121, :142-205,
 * :295-305) for consecutive frames of one stream: the dB row of the displayed slice, its auto-range over the last 20
 * frames, the normalised row and its colours. All arithmetic runs in the input's precision as numpy 2.x runs the
 * reference: float32 spectra give float32 rows, peak and floor, float64 spectra float64. The context keeps nothing
 * between calls: the caller carries the panel's state, a blob of omega_waterfall_state_size() float64 values that do
 * not depend on the slice (a validity flag, a dtype tag -- 1 for float64 --, a count, 20 dB maxima and 20 dB minima
 * oldest first with float32 values widened exactly, the current peak and floor), from state_out of one call to
 * state_in of the next; it survives a change of the slice as the reference's peak_history survives
 * set_frequency_range. state_in NULL: a new panel (peak 0, floor -80). state_out NULL: not wanted. Both live where
 * `mem` says and may be the same buffer. A blob recorded in the other precision returns OMEGA_EUNSUP: a stream has
 * one precision (for OMEGA_MEM_DEVICE the call reads the blob's head back, which waits for the context's stream).
 * One call on F frames equals F one-frame calls chained through the blob, bit for bit; n_frames 0 passes the state
 * through. The entry points are additive to ABI 5.
 * omega_waterfall_mapping: _setup_frequency_mapping (:56-69) -- freq_bins = np.linspace(0, sample_rate / 2,
 * fft_size / 2 + 1) as numpy evaluates it, first_bin = argmax(freq_bins >= min_freq), end_bin = argmax(freq_bins >=
 * max_freq) with 0 read as the last index; the row is bins [first_bin, end_bin). No context, no device.
 * omega_waterfall_configure fixes the shape and may be repeated; it needs no device. Built: n_bins
 * 1..OMEGA_WATERFALL_MAX_BINS, n_cells >= 1, first_bin >= 0, first_bin + n_cells <= n_bins; anything else returns
 * OMEGA_EUNSUP and leaves the configured shape as it was.
 * omega_waterfall_rows: frame f has its n_bins values x (float32, or float64 when f64) at spectra + f*spec_stride
 * elements; rows may overlap. Per frame: dB = 20 log10(max(x, 1e-10)) over the slice (log10 evaluated in float64
 * of the exactly widened value; for float32 input rounded to float32, then multiplied by 20 in float32), (max dB,
 * min dB) join the history, with auto_gain the peak is np.percentile(last 20 maxima, 95) and the floor
 * np.percentile(last 20 minima, 5) (method 'linear', numpy's _lerp, in the input's precision), without it the
 * carried peak and floor stay; row = clip((dB + gain_db - floor) / (peak - floor), 0, 1), zeros where peak - floor
 * is not positive.
 *   stats [n_frames, OMEGA_WATERFALL_COLS] float64:
 *     0 flags   bit 0: a non-finite bin anywhere in the frame (every other column and the row are 0, rgb holds the
 *               zero row's colours, and the frame is passed over: the state goes on as if it had not come)
 *     1 db_max, 2 db_min   of the slice
 *     3 peak, 4 floor      current_peak / current_floor after this frame
 *     5 argmax index, 6 argmax value   np.argmax over all n_bins (first occurrence) and the bin there (:302-305)
 *   rows [n_frames, n_cells] in the input's type
 *   rgb  uint8 [n_frames, n_cells, 3], or NULL (scheme is then ignored): omega_waterfall_colors of the rows
 * float64 rows agree with numpy's to 1e-12 absolute (the library's log10 against the C library's); float32 rows to
 * 8 * 2^-24 absolute (numpy's float32 log10 is not correctly rounded).
 * omega_waterfall_colors: _spectrum_to_color (:142-205) of intensities [n_rows, n_cells] (row r at intensity +
 * r*row_stride elements) -> rgb uint8 [n_rows, n_cells, 3]; needs no configuration. scheme: 0 spectrum, 1 hot,
 * 2 cool, 3 viridis (through colorsys.hsv_to_rgb), any other value the reference's grey fallback. Each component
 * is int(255 * ...), a truncation, of IEEE add / subtract / multiply / divide in the intensity's precision with the
 * literals rounded to it first, without contraction: bit for bit the reference's bytes. */
#define OMEGA_WATERFALL_COLS 7
#define OMEGA_WATERFALL_MAX_BINS 8193
#define OMEGA_WATERFALL_HISTORY 20
typedef struct {
  int32_t n_bins;     /* bins per spectrum (the app: 1025) */
  int32_t first_bin;  /* the slice's first bin (the app: 1) */
  int32_t n_cells;    /* bins in the slice (the app: 853) */
} omega_waterfall_config;
/* 1025 bins, cells [1, 854). */
void omega_waterfall_config_default(omega_waterfall_config* cfg);
int omega_waterfall_mapping(double sample_rate, int32_t fft_size, double min_freq, double max_freq, int32_t* first_bin,
                            int32_t* end_bin);
int omega_waterfall_configure(omega_ctx* ctx, const omega_waterfall_config* cfg);
/* 45; no context, no device. */
int64_t omega_waterfall_state_size(void);
int omega_waterfall_rows(omega_ctx* ctx, const void* spectra, int64_t spec_stride, int32_t f64, int64_t n_frames,
                         int32_t auto_gain, double gain_db, int32_t scheme, const double* state_in, double* state_out,
                         double* stats, void* rows, uint8_t* rgb, int mem);
int omega_waterfall_colors(omega_ctx* ctx, const void* intensity, int64_t row_stride, int32_t f64, int64_t n_rows,
                           int32_t n_cells, int32_t scheme, uint8_t* rgb, int mem);

/* ChromagramAnalyzer.detect_key / get_alternative_keys / detect_chord with the temporal blend in front of them, and
 * MusicTheory.analyze_mode for every root (omega4/panels/chromagram.py:215-339, :396-418, :670-812;
 * omega4/panels/music_theory.py:175-200) for consecutive frames of one stream, in float64. The histories, the names
 * and every rule that reads them (the flat-chroma chord fallback, the metal riff pattern, anti-stick's repeat count,
 * the history-append rule) stay with the caller (omega_gpu.ChromagramAnalyzer / ChromagramPanel). The context keeps
 * only the configuration; the caller carries the stream's state, omega_tonal_state_size() float64 values (a
 * has-previous flag and the previous frame's rolled raw row), from state_out of one call to state_in of the next.
 * state_in NULL: no predecessor. state_out NULL: not wanted. Both live where `mem` says and may be the same buffer.
 * One call on F frames equals F one-frame calls chained through the blob, bit for bit; n_frames 0 passes the state
 * through. The entry points are additive to ABI 5.
 * omega_tonal_configure fixes the genre (omega_tonal_genre; any other value returns OMEGA_EINVAL and leaves the
 * configuration as it was) and may be repeated; it needs no device. `other` is what the reference does for a genre
 * name it does not know: pop's weights and tolerance, the pop / classical chord types, threshold 0.03, blend 0.3,
 * no key factor and no chord bonus. The blend factor is 0.7 for metal and rock, 0.5 for jazz, else 0.3.
 * omega_tonal_features: raw_chroma [n_frames, 12] float64 as omega_chroma writes it (smoothed, normalised, not yet
 * blended). roll [n_frames] int32 or NULL (0): the frame's tuning offset in semitones, -11..11, applied as
 * np.roll(row, roll); a value outside returns OMEGA_EINVAL before anything is launched (for OMEGA_MEM_DEVICE the
 * array is read back first, which waits for the context's stream). first [n_frames] int32 or NULL (0): non-zero
 * marks a frame without predecessor (it stays unblended, whatever the carry holds). Per frame: blended =
 * prev * (1 - a) + cur * a of the rolled rows, then
 *   rows [n_frames, OMEGA_TONAL_COLS] float64:
 *     0..11  the blended chroma
 *     12     flags: bit 0 a non-finite value (the frame is scored as the all-zero row), bit 1 np.sum == 0,
 *            bit 2 np.var < 0.001
 *     13     np.var of the blended chroma
 *     14, 15 the key: index 2 root + (1 for minor) and its adjusted correlation (the first maximum, :331)
 *     16..18, 19..21  the three best alternative keys by a stable descending sort (:417): indices, correlations
 *     22, 23 the chord: cell 13 root + type in chord_types order, -1 for N/A, and its score (:754)
 *     24..27 anti-stick (:781-818; metal and rock only, else -1 / 0): first index, first score, second index,
 *            second score of a stable descending sort of the second matrix
 *     28..39, 40..51  analyze_mode for root 0..11: the mode's index in MusicTheory.MODES order, and its score
 *   key_corr [n_frames, 24], alt_corr [n_frames, 24] (index 2 root + minor), chord [n_frames, 2, 12, 13] (matrix 0
 *   detect_chord's scores, matrix 1 the anti-stick variant; NaN where a cell is not tested), mode [n_frames, 12, 7]:
 *   the scores behind the decisions; each may be NULL.
 * Correlations and chord scores agree with numpy's to 1e-12 absolute.
 * omega_tonal_spectra: the same from magnitude spectra [n_frames, n_bins] float32, contiguous, with omega_chroma's
 * limits (n_bins >= 3, df > 0): omega_chroma's kernel writes the raw rows into context scratch and the tonal kernel
 * runs behind it on the context's stream; nothing returns to the host in between. */
#define OMEGA_TONAL_COLS 52
typedef enum {
  OMEGA_TONAL_POP = 0, OMEGA_TONAL_JAZZ = 1, OMEGA_TONAL_CLASSICAL = 2, OMEGA_TONAL_METAL = 3, OMEGA_TONAL_ROCK = 4,
  OMEGA_TONAL_OTHER = 5
} omega_tonal_genre;
typedef struct {
  int32_t genre; /* omega_tonal_genre */
} omega_tonal_config;
/* pop. */
void omega_tonal_config_default(omega_tonal_config* cfg);
int omega_tonal_configure(omega_ctx* ctx, const omega_tonal_config* cfg);
/* 13; no context, no device. */
int64_t omega_tonal_state_size(void);
int omega_tonal_features(omega_ctx* ctx, const double* raw_chroma, int64_t n_frames, const int32_t* roll,
                         const int32_t* first, const double* state_in, double* state_out, double* rows,
                         double* key_corr, double* alt_corr, double* chord, double* mode, int mem);
int omega_tonal_spectra(omega_ctx* ctx, const float* spectra, int64_t n_frames, int32_t n_bins, double df,
                        const int32_t* roll, const int32_t* first, const double* state_in, double* state_out,
                        double* rows, double* key_corr, double* alt_corr, double* chord, double* mode, int mem);

/* ProfessionalMetersPanel.update (omega4/panels/professional_meters.py:348-397, with :554-579) for consecutive frames
 * of one stream: what the panel does with a frame and with the five values calculate_lufs returned for it -- the
 * level, true-peak and loudness-range histories, the level histogram, the peak hold and the "simple transient
 * detection". The metering itself is omega_calculate_lufs; its meters rows are this call's input. The context keeps
 * only the configured shape; the caller carries the panel's state, omega_meterpanel_state_size(cfg) float64 values:
 *   0 hold value, 1 hold counter, 2 attack_time, 3 punch_factor, 4 transients_detected, 5 / 6 the level ring's fill
 *   and next slot, 7 / 8 the true-peak ring's, 9 / 10 the range ring's, 11..15 zero, then the three rings (level_len,
 *   peak_len, range_len values; a ring fills from slot 0 and then wraps)
 * from state_out of one call to state_in of the next. state_in NULL: a new panel (hold -100 / 0, transient values 0,
 * empty histories). state_out NULL: not wanted. Both live where `mem` says and may be the same buffer. One call on F
 * frames equals F one-frame calls chained through the blob, bit for bit; n_frames 0 writes state_in's panel (with
 * reset_hold applied) to state_out. The entry points are additive to ABI 5.
 * omega_meterpanel_state_size, omega_meterpanel_edges and omega_meterpanel_unpack need no context and no device.
 * They, and omega_meterpanel_configure, return OMEGA_EINVAL for a sample rate that is not positive and finite, a
 * negative frame_len, a history length outside 1..OMEGA_METERPANEL_MAX_HISTORY, n_bins outside
 * 1..OMEGA_METERPANEL_MAX_BINS, hist_lo / hist_hi not finite or not increasing (or so close that two edges
 * coincide), and OMEGA_EUNSUP for frame_len 0 or above OMEGA_METERPANEL_MAX_FRAME; a refused configure leaves the
 * configured shape as it was. omega_meterpanel_edges writes the n_bins + 1 histogram edges, np.linspace(hist_lo,
 * hist_hi, n_bins + 1) as numpy evaluates it; the device searches this very table. omega_meterpanel_unpack reads a
 * blob in host memory: the three histories oldest first (level_len / peak_len / range_len values of room each) with
 * their lengths, hold[2] = value, counter and transient[3] = attack_time, punch_factor, transients_detected; every
 * output may be NULL; a blob whose fills and slots are not a ring's returns OMEGA_EINVAL and writes nothing.
 * omega_meterpanel_update: frame f has its frame_len samples (float32, or float64 when f64) at frames +
 * f*frame_stride, in elements; rows may overlap. meters [n_frames, 5] float64 as omega_calculate_lufs writes them
 * (momentary, short_term, integrated, range, true_peak). peak_hold_samples is the panel's attribute at these frames;
 * reset_hold non-zero applies reset_peak_hold before the first frame. Per frame, in order: the histories take
 * momentary, range and true_peak; the hold takes true_peak and the counter peak_hold_samples where true_peak > hold,
 * else the counter drops by one and at <= 0 the hold takes true_peak (the counter runs negative without bound); and,
 * in the frame's dtype, d = diff(|x|): where any d > 0.1 (float32 frames: against float32(0.1)), attack_time =
 * (first such index / sample_rate) * 1000, punch_factor = max|x| / sqrt(mean(x^2)) with numpy's pairwise sum and a
 * correctly rounded divide (0 unless the rms is > 0), transients_detected = their number; where none, the three keep
 * the frame before's. NaN follows numpy: np.max propagates it and every comparison with it is false.
 *   rows [n_frames, OMEGA_METERPANEL_COLS] float64:
 *     0 hold value   1 hold counter   2 attack_time in ms   3 punch_factor   4 transients_detected
 *     5 flags: bit 0 an attack in this frame, bit 1 a non-finite sample in it
 *     6 the level history's fill   7 the histogram's sum
 *   hist [n_frames, n_bins] int32 or NULL: np.histogram(level_history, edges) after frame f -- bin b holds
 *     edges[b] <= v < edges[b + 1], the last bin also v == edges[n_bins], every other value (NaN, -100) nowhere
 * Float32 frames give numpy's bits in every column; float64 frames differ from numpy in the punch factor alone, by
 * the rounding of the square root and the divide (1e-12 relative at the very most). */
#define OMEGA_METERPANEL_COLS 8
#define OMEGA_METERPANEL_MAX_BINS 62
#define OMEGA_METERPANEL_MAX_HISTORY 4096
#define OMEGA_METERPANEL_MAX_FRAME 16384
typedef struct {
  double sample_rate;
  int32_t frame_len;   /* samples per audio frame, 1..16384 (1: the meters part only, as the reference's len > 1) */
  int32_t level_len;   /* level_history's maxlen */
  int32_t peak_len;    /* true_peak_history's */
  int32_t range_len;   /* loudness_range_history's */
  int32_t n_bins;      /* histogram bins */
  double hist_lo, hist_hi;
} omega_meterpanel_config;
/* 48000 Hz, 2048 samples, 600 / 300 / 300, 60 bins over -60..0. */
void omega_meterpanel_config_default(omega_meterpanel_config* cfg);
int64_t omega_meterpanel_state_size(const omega_meterpanel_config* cfg);
int omega_meterpanel_edges(const omega_meterpanel_config* cfg, double* out);
int omega_meterpanel_unpack(const omega_meterpanel_config* cfg, const double* state, double* level, int32_t* n_level,
                            double* peaks, int32_t* n_peaks, double* ranges, int32_t* n_ranges, double* hold,
                            double* transient);
int omega_meterpanel_configure(omega_ctx* ctx, const omega_meterpanel_config* cfg);
int omega_meterpanel_update(omega_ctx* ctx, const void* frames, int64_t frame_stride, int32_t f64, const double* meters,
                            int64_t n_frames, int64_t peak_hold_samples, int32_t reset_hold, const double* state_in,
                            double* rows, int32_t* hist, double* state_out, int mem);

/* ---- Sustained-stream ingest ------------------------------------------
 * The capture byte stream of omega4/audio/capture.py:546-600 (parec float32le / s16le, fixed chunks
 * of chunk_size samples, s16 scaled by 1/32768), its per-chunk noise gate (:620-641: RMS, background
 * EMA, silence counter -> zeros) and the app's input gain + ring buffer (omega4_main.py:648-688),
 * feeding omega_process_stream: frame f of every channel covers stream samples [f*hop, f*hop + W).
 * Bytes are interleaved over the context's n_channels. The gate works as the reference's capture
 * loop does for any channel count: a chunk is chunk_size interleaved samples (capture.py:549-550,
 * chunk_size / C frames), one RMS over all its channels, one background level and one silence
 * counter (+chunk_size per quiet chunk) for the stream, a gated chunk zeroes every channel of it.
 * The gate's float32 arithmetic is numpy >= 2's (NEP 50: a Python float times a float32 scalar stays
 * float32; the golden vectors were recorded with numpy 2.2.6). omega_ingest_push memcpy's them into
 * page-locked staging slots; each full slot (batch_hops * hop samples per channel) is copied to the
 * device on a copy stream and analysed on the ingest's compute stream (bound to the context with
 * omega_set_stream; destroy the ingest before the context, and before using the context directly
 * again), overlapping the next slot's copy. push blocks only while the slot it fills is still being
 * copied to the device. Results come back through omega_ingest_poll in frame order; when
 * max_pending_batches batches wait unpolled, the oldest one's frames are dropped and counted (the
 * capture buffer's drop policy, capture.py:579-580). */
typedef enum { OMEGA_FMT_F32LE = 0, OMEGA_FMT_S16LE = 1 } omega_sample_format;
enum { OMEGA_INGEST_COMBINED = 1, OMEGA_INGEST_LUFS = 2, OMEGA_INGEST_TRUE_PEAK = 4, OMEGA_INGEST_METERS = 8 };

typedef struct {
  int32_t format;                   /* omega_sample_format */
  int32_t sample_rate;              /* for the gate's silence threshold (capture.py:227) */
  int32_t hop;                      /* frame hop H, multiple of 4 */
  int32_t batch_hops;               /* hops per device batch; batch_hops * hop * n_channels % chunk_size == 0 */
  int32_t ring_slots;               /* page-locked input staging slots, >= 2 */
  int32_t max_pending_batches;      /* result blocks kept until polled (>= 2); beyond, the oldest drop */
  int32_t chunk_size;               /* capture chunk (noise-gate block), 1..8192 (capture.py:28, :64) */
  float gain;                       /* input_gain (omega4_main.py:152, :660) */
  int32_t gate;                     /* apply the capture noise gate */
  double noise_floor;               /* 0.001 (capture.py:36) */
  double silence_threshold_seconds; /* 0.25 */
  double background_alpha;          /* 0.001 */
  int32_t want;                     /* OMEGA_INGEST_* outputs */
} omega_ingest_config;

typedef struct {
  int64_t bytes_in, batches, frames, frames_polled, dropped_frames;
} omega_ingest_stats;

typedef struct omega_ingest omega_ingest;

void omega_ingest_config_default(omega_ingest_config* cfg);
/* On an error after allocation *out is set: read omega_ingest_last_error, then omega_ingest_destroy. */
int omega_ingest_create(omega_ctx* ctx, const omega_ingest_config* cfg, omega_ingest** out);
int omega_ingest_push(omega_ingest* in, const void* bytes, int64_t n_bytes);
/* Analyse the whole capture chunks buffered so far in whole frames (the rest stays buffered). */
int omega_ingest_flush(omega_ingest* in);
/* Up to max_frames completed frames (per channel) in frame order into host buffers laid out like
 * omega_outputs ([frames * C, T], [frames * C], [frames * C, 5]; NULL pointers skip); wait != 0
 * blocks until the launched batches are done. */
int omega_ingest_poll(omega_ingest* in, int64_t max_frames, const omega_outputs* out, int wait, int64_t* n_frames_out);
int omega_ingest_get_stats(const omega_ingest* in, omega_ingest_stats* out);
const char* omega_ingest_last_error(const omega_ingest* in);
void omega_ingest_destroy(omega_ingest* in);

#ifdef __cplusplus
}
#endif
#endif /* OMEGA_H */
