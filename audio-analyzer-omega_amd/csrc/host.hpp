// libomega.so host side, private header: the context behind the C ABI of include/omega.h, the kernel
// launchers' prototypes and the helpers the capi_*.cpp translation units share. Everything in
// omega_host is hidden from the library's dynamic symbol table.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <new>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/omega.h"
#include "batch_plan.hpp"
#include "design.hpp"
#include "meter_sync.hpp"
#include "params.hpp"

namespace omega {
hipError_t launch_mrfft(const SpectralParams& p, hipStream_t s);
hipError_t launch_mrfft_independent(const SpectralParams& p, hipStream_t s);
hipError_t launch_truepeak(int W, const SpectralParams& p, hipStream_t s);
hipError_t launch_truepeak_rf(int W, const SpectralParams& p, hipStream_t s, int extra_lds = 0);
hipError_t launch_mrfft_rf(int n, const SpectralParams& p, int r, hipStream_t s);
hipError_t launch_rfft(int m, const RfftParams& p, hipStream_t s);
hipError_t launch_kweight(int m, const KWeightParams& p, hipStream_t s);
hipError_t launch_weight64(const Weight64Params& p, hipStream_t s);
hipError_t launch_any(const AnyFftParams& p, int truepeak, hipStream_t s);
hipError_t launch_spectra(int m, const SpectraParams& p, int grid, hipStream_t s);
hipError_t launch_spectra_rf(int m, const SpectraParams& p, hipStream_t s);
hipError_t launch_meter_prep(const MeterPrepParams& p, hipStream_t s);
hipError_t launch_meter_query(const MeterPrepParams& p, hipStream_t s);
hipError_t launch_meter_load(const MeterLoadParams& p, hipStream_t s);
hipError_t launch_queue_probe(unsigned* w, unsigned target, int limit, hipStream_t side, hipStream_t main);
hipError_t launch_bands(const BandParams& p, hipStream_t s);
hipError_t launch_chroma(const float* spec, int64_t n, int n_bins, int lo, int hi, const double* mat, double* out,
                         hipStream_t s);
hipError_t launch_combine(const CombineParams& p, hipStream_t s);
hipError_t launch_drum(const DrumParams& p, hipStream_t s);
hipError_t launch_vu(const VuParams& p, hipStream_t s);
hipError_t launch_transients(const TransientParams& p, hipStream_t s);
hipError_t launch_transients_any(const TransientParams& p, hipStream_t s);
hipError_t launch_post(const PostParams& p, hipStream_t s);
hipError_t launch_pitch(const PitchParams& p, hipStream_t s);
hipError_t launch_harmonic(const HarmonicParams& p, hipStream_t s);
hipError_t launch_genre(const GenreParams& p, hipStream_t s);
hipError_t launch_hiphop(const HipHopParams& p, hipStream_t s);
hipError_t launch_phase(const PhaseParams& p, hipStream_t s);
hipError_t launch_room_modes(const RoomModesParams& p, hipStream_t s);
hipError_t launch_room_rt60(const RoomRt60Params& p, hipStream_t s);
hipError_t launch_voice(const VoiceParams& p, hipStream_t s);
hipError_t launch_tdetect(const TdetectParams& p, hipStream_t s);
hipError_t launch_rhythm(const RhythmParams& p, hipStream_t s);
hipError_t launch_basszoom_frames(const BassZoomParams& p, hipStream_t s);
hipError_t launch_basszoom_track(const BassZoomParams& p, hipStream_t s);
hipError_t launch_waterfall(const WaterfallParams& p, hipStream_t s);
hipError_t launch_waterfall_colors(const WaterfallColorParams& p, hipStream_t s);
hipError_t launch_tonal(const TonalParams& p, hipStream_t s);
hipError_t launch_meterpanel_frames(const MeterPanelParams& p, int wave_max, hipStream_t s);
hipError_t launch_meterpanel_track(const MeterPanelParams& p, bool walk, hipStream_t s);
hipError_t launch_batch(const SpectralParams& sp, const KWeightParams& kp, const BatchPlan& bp, const MeterPrepParams& mp,
                        int grid, hipStream_t s);
}  // namespace omega

using namespace omega;

namespace omega_host __attribute__((visibility("hidden"))) {

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
};

struct HostOut {  // one output of a host-memory call
  void* host;
  void* dev;
  size_t bytes;
  size_t arena_off;  // offset in the output arena, or ~0 (a slot of its own)
};

// ---- per-family context state: one sub-struct of omega_ctx per feature family ----

// capi_spectrum.cpp -- drum-feature stream state (omega_drum_features), double-buffered, for `bins` bins
// per frame
struct DrumState {
  int bins = 0, cur = 0;
  float* prev[2] = {};
  float* hist[2] = {};
  int* len[2] = {};
  long long* pos[2] = {};
  float* flux = nullptr;
  int64_t flux_cap = 0;  // (elements)
};

// capi_spectrum.cpp -- post-processing
struct PostState {
  PostParams p{};  // omega_post_configure's tables (p.T = 0: not configured)
  float* raw = nullptr;  // post-processing band scratch (pre-EMA values)
  int64_t raw_cap = 0;
};

// capi_time.cpp -- VU meter state (omega_vu_update), double-buffered: sample history, display / peak /
// hold time
struct VuState {
  double* hist[2] = {};
  double* st[2] = {};
  double* ms = nullptr;
  int64_t ms_cap = 0, total = 0;
  int cur = 0;
};

// capi_time.cpp -- transient analysis: the plans of the lengths that are no power of two up to 8192 (the
// radices and, beside them, e^{-2 pi i m / n} in float64) and the global work buffer of the longest
struct TransientState {
  std::map<int, std::pair<std::vector<int>, double2*>> any;
  double2* scratch = nullptr;
  int64_t scratch_cap = 0;
};

// capi_time.cpp -- pitch detection (omega_pitch_configure / omega_pitch_detect): the configuration with
// its derived periods and high-pass sections
struct PitchState {
  bool set = false;
  PitchParams p{};
};

// capi_time.cpp -- stereo phase correlation (omega_phase_configure / omega_phase_correlation): the
// configuration with the band ranges (no frame state)
struct PhaseState {
  bool set = false;
  PhaseParams p{};
};

// capi_room.cpp -- room acoustics (omega_room_configure / omega_room_modes / omega_room_decay): the
// configuration with the in-range bins and the uploaded frequency table (no frame state)
struct RoomState {
  bool set = false;
  RoomModesParams p{};
  double fs = 0.0;
  double* freqs = nullptr;
  int64_t freqs_cap = 0;
};

// capi_voice.cpp -- voice detection (omega_voice_configure / omega_voice_features): the configuration with the
// voice bin range and the lag range (no frame state)
struct VoiceState {
  bool set = false;
  VoiceParams p{};
};

// capi_tdetect.cpp -- transient detection (omega_tdetect_configure / omega_tdetect_features): the configuration
// with the band indices and the high-pass design (the stream state travels with the caller), the lfilter
// carry-scan table per (sample rate, frame length), the per-call workspace and the two state blobs that chain a
// call's launches
struct TdetectState {
  bool set = false;
  TdetectParams p{};
  std::map<std::pair<double, int>, TdScan*> scans;
  double* ws = nullptr;
  int64_t ws_cap = 0;
  double* chain[2] = {};
};

// capi_basszoom.cpp -- the bass zoom panel (omega_basszoom_configure / omega_basszoom_features): the configuration
// with the bar mapping (the panel's state travels with the caller)
struct BassZoomState {
  bool set = false;
  BassZoomParams p{};
};

// capi_rhythm.cpp -- beat detection and band tracking (omega_rhythm_configure / omega_rhythm_features): the
// configuration with the edges, the uploaded frequency table and the host's copy of it (an unchanged table is not
// uploaded again), the per-call flag workspace and the two state blobs that chain a call's launches (the stream
// state travels with the caller)
struct RhythmState {
  bool set = false;
  RhythmParams p{};
  double* freqs = nullptr;
  int64_t freqs_cap = 0;
  std::vector<double> freqs_host;
  int* ws = nullptr;
  int64_t ws_cap = 0;
  double* chain[2] = {};
};

// capi_waterfall.cpp -- the spectrogram waterfall (omega_waterfall_configure / omega_waterfall_rows): the configured
// shape and the two state blobs that chain a call's launches (the panel's state travels with the caller)
struct WaterfallState {
  bool set = false;
  int n_bins = 0, first_bin = 0, n_cells = 0;
  double* chain[2] = {};
};

// capi_tonal.cpp -- key, chord and mode scores (omega_tonal_configure / omega_tonal_features / omega_tonal_spectra):
// the configured genre, the raw chroma rows omega_tonal_spectra keeps on the device between its two kernels, and
// the two state blobs that chain a call's launches (the stream's state travels with the caller)
struct TonalState {
  bool set = false;
  int genre = 0;
  double* raw = nullptr;
  int64_t raw_cap = 0;
  double* chain[2] = {};
};

// capi_meterpanel.cpp -- the professional meters panel (omega_meterpanel_configure / omega_meterpanel_update): the
// configured shape with the uploaded edges, the [hist_lo, hist_hi] pairs whose edges are in omega_ctx::tables, and
// the frame kernel's per-call records (the panel's state travels with the caller)
struct MeterPanelState {
  bool set = false;
  MeterPanelParams p{};
  int64_t state_len = 0;
  std::vector<std::pair<double, double>> ranges;
  double* ws = nullptr;
  int64_t ws_cap = 0;
};

// capi_features.cpp -- the stream state of a feature that compares each frame's spectrum with the one
// before (harmonic, genre): the frequency table and the previous frame's spectrum, double-buffered (a
// launch reads prev[cur] and writes prev[cur ^ 1])
struct PrevSpectrum {
  double* freqs = nullptr;
  float* prev[2] = {};
  int cur = 0;
  bool has_prev = false;
  // prev_in / prev_out of the launch over frames [f0, f0 + count) of a call's n_frames spectra at `spec`
  void chunk(const Rows32& spec, int64_t f0, int64_t count, int64_t n_frames, const float** in, float** out) const {
    *in = f0 ? spec.row(f0 - 1) : (has_prev ? prev[cur] : nullptr);
    *out = f0 + count == n_frames ? prev[cur ^ 1] : nullptr;
  }
  void advance() {
    cur ^= 1;
    has_prev = true;
  }
};

// capi_features.cpp -- harmonic analysis (omega_harmonic_configure / omega_harmonic_analyze): the
// configuration, the stream state and np.hamming per audio length -- a bounded map of its own, emptied when
// full (harmonic_window), and so kept out of omega_ctx::tables, whose entries are never freed
struct HarmonicState {
  bool set = false;
  HarmonicParams p{};
  PrevSpectrum stream;
  std::map<int, double*> ham;
};

// capi_features.cpp -- genre features (omega_genre_configure / omega_genre_features): the configuration
// with the band ranges, and a stream state of its own
struct GenreState {
  bool set = false;
  GenreParams p{};
  PrevSpectrum stream;
};

// capi_features.cpp -- hip-hop features (omega_hiphop_configure / omega_hiphop_features): the
// configuration with the band ranges and the three band-pass cascades (no frame state) and the designed
// sections as scipy lays them out
struct HipHopState {
  bool set = false;
  HipHopParams p{};
  double sos[3][4][6] = {};
};
}  // namespace omega_host

using namespace omega_host;

struct omega_bands {
  omega_ctx* ctx;
  int op, n_bands, n_out, n_bins, n_valid;
  int32_t* d_starts;
  int32_t* d_ends;
  float* d_scale;
  float* d_bin_scale;
};

struct omega_ctx {
  omega_config cfg{};
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  // fork/join streams + events for the concurrent branches, and the graph cache
  hipStream_t cap = nullptr, fork[1] = {nullptr};
  std::vector<hipStream_t> spare;  // side streams found on the context stream's hardware queue (kept
                                   // alive so the next one created lands on another queue; at most
                                   // kMaxSpare, the oldest destroyed beyond that)
  unsigned* d_probe = nullptr;     // side_stream_check's two words
  unsigned probe_seq = 0;
  std::vector<hipStream_t> checked;  // streams probed against the current fork[0] (cleared when it changes)
  bool queue_shared = false;         // the last probe found no independent queue for fork[0]
  hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  // HIP graph replay of device-memory calls: off by default -- on MI355X (ROCm 7) a replayed graph
  // put the stream layout's nodes on other queues, with ~12 us cross-queue waits and ~20 us between
  // consecutive launches (cfg2 step 149.5 us vs 128.8 us for direct launches of the same layout)
  bool use_graph = false;
  // stream layout of the per-batch work (enqueue_frames): 3 (default; 16384-sample frames, direct
  // launches) one batch_kernel launch for all per-channel-frame work, the meter prep on the side stream
  // waiting on the batch's K-weighting count (kw_done) instead of a stream event; 2 (other frame sizes,
  // graph capture, or omega_set_graphs layout bits) the full-chip kernels back to back with the meter
  // aggregates on a side stream joined by events.
  int layout = 3;
  // the device counter words (meter_sync.hpp: MeterCounter) and the host's ledger of what was launched to
  // count into them, with the side stream's unjoined-meter-work flag; every transition is a step function
  // there, the table is in DESIGN.md §4
  unsigned* d_ctr = nullptr;
  MeterSync ms;
  // meter pipelining (omega_set_meter_pipelining): the params of the pending segment (MeterSync::pend)
  bool pipe = false;
  MeterPrepParams pend_mq{};
  int stage_par = 0;  // pipelined calls alternate the staging of LUFS_inst / TP (the segment reads them later)
  // pipelined launches: the signal-memory word the grid's last-dispatched workgroup bumps, for the side
  // stream's hipStreamWaitValue32 before the prep (tail_ok: 1 ready, -1 not supported, no wait), and the
  // K-weighting workgroups' {generation, LUFS} words, two parities of kMeterChunk x C
  unsigned* d_tail = nullptr;
  unsigned long long* d_mirror = nullptr;
  int tail_ok = 0;
  // overlapped pipelined batches (omega_set_meter_pipelining, with tail_ok > 0): call i's batch launch
  // and, behind it, its meter segment as a launch of its own go to bs[i & 1] (two non-blocking streams,
  // created when pipelining is first enabled), batch i gated on batch i - 1's tail count; ev_done[k]
  // follows the segment on bs[k], and the caller's stream waits for call i's only in call i + 1 (or a
  // flush): `unjoined` = the call on bs[last_bs] is not yet ordered into the caller's stream.
  // prev_span: what that call reads ([0]) and writes (the rest) -- a call touching any of it runs serial
  hipStream_t bs[2] = {nullptr, nullptr};
  hipEvent_t ev_in = nullptr, ev_done[2] = {nullptr, nullptr};
  unsigned bs_idx = 0;
  int last_bs = 0;
  bool unjoined = false;
  bool bs_shared = false;  // the last probe left a batch stream on a shared hardware queue (calls serialise)
  std::vector<std::pair<const char*, size_t>> prev_span;
  // device-side poll expiry flags (host-mapped: [0] meter prep, [1] join), checked by
  // check_device_err; the poll bound (OMEGA_POLL_LIMIT, a test knob)
  unsigned* h_err = nullptr;
  unsigned* d_err = nullptr;
  int poll_limit = 1 << 22;
  float* d_lufs_scr = nullptr;  // omega_calculate_lufs: instantaneous values kept on the device
  int64_t lufs_scr_cap = 0;
  bool res_independent = false;  // no combine target has several owners: resolution kernels commute
  hipEvent_t ev_kw = nullptr;
  struct GraphEntry {
    std::vector<uint64_t> key;
    hipGraph_t graph;
    hipGraphExec_t exec;
  };
  std::vector<GraphEntry> graphs;
  char err[512] = {};  // omega_last_error (a fixed buffer: reporting an error allocates nothing)
  // tables
  float2* d_tw[kMaxLog2] = {};

  float2* d_rot = nullptr;
  float* d_win[kMaxRes] = {};
  float* d_wgt[kMaxRes] = {};
  CombEnt* d_ent = nullptr;
  int ent_begin[kMaxRes] = {}, ent_end[kMaxRes] = {};
  int pair_lo[kMaxRes] = {}, pair_hi[kMaxRes] = {};  // ResParam::pair_lo / pair_hi
  int ent_jmax[kMaxRes] = {};  // the highest bin a resolution's combine entries read (j + 1)
  std::map<std::pair<int, int>, BiquadTab*> kw_tabs;  // (M, chunk) -> device {hp, shelf}
  int rf_sizes = 1 << 14;   // resolution sizes on the register-FFT kernel (bit log2 N): the 16384-point one
  std::map<std::pair<int, int>, float*> windows;  // (m, kind) -> device window
  std::map<int, float2*> rots;                     // m -> true-peak rotation table
  // the feature families' float64 tables (get_twiddles64 / get_window64 / get_savgol below), each under
  // (its kind, its two parameters). Entries are never evicted: the configured params (phase.p.tw,
  // tdetect.p.tw_*, basszoom.p.win, voice.p.sg, ...) hold these pointers between calls.
  std::map<std::tuple<int, int, int>, void*> tables;
  // combine plan as per-target owner lists (CSR) for omega_combine over a subset of resolutions
  int* d_own_off = nullptr;
  int* d_own_rj = nullptr;  // (r << 24) | j
  float* d_own_frac = nullptr;
  std::map<int, std::pair<double*, std::pair<int, int>>> chroma_mats;  // n_bins -> (mat, [lo, hi))
  double chroma_df = 0.0;
  // compact chromagram tables of omega_spectra, per (n_bins, df): 5 float32 weights per bin, bins
  // grouped by base pitch class
  struct ChromaTab {
    int n_bins = 0, lo = 0, hi = 0;
    double df = 0.0;
    float4* w4 = nullptr;
    float* w1 = nullptr;
    unsigned short* perm = nullptr;
    int* goff = nullptr;
    float* rec = nullptr;
  } ctab;
  int n_cu = 0;
  // per-family state (the structs above, each beside its family's file name)
  DrumState drum;
  PostState post;
  VuState vu;
  TransientState tr;
  PitchState pitch;
  HarmonicState harm;
  GenreState genre;
  HipHopState hiphop;
  PhaseState phase;
  RoomState room;
  VoiceState voice;
  TdetectState tdetect;
  BassZoomState basszoom;
  RhythmState rhythm;
  WaterfallState waterfall;
  TonalState tonal;
  MeterPanelState meterpanel;
  // omega_weighting: float64 filter cascades per mode and the per-launch working buffers
  W64Stage* w64[4] = {};
  // frames of any length (anyfft.hip): per N the radices and the twiddle / rotation tables
  struct AnyPlan {
    std::vector<int> radix;
    float2* tw = nullptr;
    double2* tw64 = nullptr;
    float2* rot = nullptr;
  };
  std::map<int, AnyPlan> any_plans;
  float2* d_any = nullptr;
  int64_t any_cap = 0;
  double* d_w64 = nullptr;
  int64_t w64_cap = 0;
  // meter state (double-buffered)
  float* d_hist_l[2] = {};
  float* d_hist_t[2] = {};
  int* d_nl[2] = {};
  int* d_nt[2] = {};
  unsigned long long* d_skeys[2] = {};  // sorted gated history keys (double-buffered state)
  int* d_ns[2] = {};
  uint32_t* d_t0[2] = {};
  // per-batch meter scratch, two sets by the state's parity (MeterSync::cur): the next batch's prep writes the
  // other set from before its K-weighting values are in, while this batch's queries read this one
  float* d_core[2] = {nullptr, nullptr};
  MeterExt* d_ext[2] = {nullptr, nullptr};
  int* d_ncore[2] = {nullptr, nullptr};
  int* d_next[2] = {nullptr, nullptr};
  int* d_gcount[2] = {nullptr, nullptr};
  double* d_gsum[2] = {nullptr, nullptr};
  int HL = 0, HT = 0;
  // staging for OMEGA_MEM_HOST: device slots, page-locked host slots for the inputs, and one device +
  // page-locked output arena per call (every output of a call comes back in one D2H copy)
  std::vector<DevBuf> stage;
  std::vector<DevBuf> pin;
  DevBuf oarena, oarena_pin;
  size_t oarena_used = 0, oarena_want = 0;  // the device output arena's use in this call, its wanted size
  size_t zc_used = 0;                       // the zero-copy output buffer's use in this call
  // the call's outputs may be written by the kernels straight into the page-locked arena (set by calls
  // whose kernels only store their outputs: no output is read back by another workgroup)
  bool zc_ok = false;
  DevBuf zc_pin;
  void* zc_dev = nullptr;
  std::vector<void*> allocs;
};

namespace omega_host __attribute__((visibility("hidden"))) {

// ---- errors (capi_core.cpp) ----
int fail(omega_ctx* c, int code, const char* fmt, ...);
int guard_fail(omega_ctx* c) noexcept;

#define HIPC(ctx, x)                                                                           \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) return fail(ctx, OMEGA_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

// frees an allocation tracked in omega_ctx::allocs now (null tolerated); its streams are idle already
void release(omega_ctx* c, void* p);

template <class T>
int dalloc(omega_ctx* c, T** p, size_t count) {
  void* q = nullptr;
  const hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
  if (e != hipSuccess) return fail(c, OMEGA_ENOMEM, "hipMalloc(%zu): %s", count * sizeof(T), hipGetErrorString(e));
  c->allocs.push_back(q);
  *p = static_cast<T*>(q);
  return 0;
}

// A per-call scratch buffer of at least `need` elements: grown by replacement (the old buffer freed
// once this context's streams are idle -- work already enqueued may still read it; other contexts and
// streams on the device are not waited for), so repeated calls with growing sizes keep one buffer
// instead of accumulating them until omega_destroy.
template <class T>
int grow(omega_ctx* c, T** p, int64_t* cap, int64_t need) {
  if (need <= *cap) return 0;
  if (*p) {
    HIPC(c, hipStreamSynchronize(c->stream));
    for (hipStream_t f : c->fork)
      if (f) HIPC(c, hipStreamSynchronize(f));
    for (hipStream_t f : c->bs)  // (an overlapped pipelined batch may still run there)
      if (f) HIPC(c, hipStreamSynchronize(f));
    release(c, *p);
    *p = nullptr;
    *cap = 0;
  }
  if (int e = dalloc(c, p, (size_t)need)) return e;
  *cap = need;
  return 0;
}

template <class T>
int upload(omega_ctx* c, T** p, const std::vector<T>& v) {
  int r = dalloc(c, p, v.size());
  if (r) return r;
  HIPC(c, hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// A device table kept in map `m` under `key`: built and uploaded by build(&table) on first use.
template <class M, class K, class B>
int cached(M& m, const K& key, typename M::mapped_type* out, B build) {
  auto it = m.find(key);
  if (it == m.end()) {
    typename M::mapped_type d{};
    if (int e = build(&d)) return e;
    it = m.emplace(key, d).first;
  }
  *out = it->second;
  return 0;
}

// A float64 table of omega_ctx::tables: built by build() and uploaded on first use, freed at omega_destroy
template <class T, class B>
int host_table(omega_ctx* c, int kind, int a, int b, const T** out, B build) {
  void* d = nullptr;
  if (int e = cached(c->tables, std::make_tuple(kind, a, b), &d, [&](void** p) {
        T* t = nullptr;
        const int r = upload(c, &t, build());
        *p = t;
        return r;
      }))
    return e;
  *out = static_cast<const T*>(d);
  return 0;
}
// e^{-2 pi i q / period}, q < count (design.hpp twiddles64). Keyed by what the caller asks for: families that
// read a prefix of one period's table ask for the common count, period / 2 + 1, and share one upload.
inline int get_twiddles64(omega_ctx* c, int period, int count, const double2** out) {
  return host_table(c, 0, period, count, out, [&] { return twiddles64(period, count); });
}
// np.blackman / np.hanning / np.hamming (M) in float64 (design.hpp np_window64; kind: OMEGA_WIN_*)
inline int get_window64(omega_ctx* c, int kind, int M, const double** out) {
  return host_table(c, 1, kind, M, out, [&] { return np_window64(kind, M); });
}
// the w x w Savitzky-Golay cubic weights (design.hpp savgol_cubic)
inline int get_savgol(omega_ctx* c, int w, const double** out) {
  return host_table(c, 2, w, 0, out, [&] {
    std::vector<double> W((size_t)w * w);
    savgol_cubic(w, W.data());
    return W;
  });
}

// ---- the side stream (omega_ctx::fork[0]: the latency-bound meter kernels and omega_calculate_lufs' true
// peak, beside the caller's stream) and its two event orders. Which way each orders reads off its name; the
// ledger (MeterSync::side) records that a meter kernel went there and that the caller's stream joined it. ----
inline hipStream_t side_stream(const omega_ctx* c) { return c->fork[0]; }
// `waiter` runs after everything enqueued on the caller's stream so far (ev_fork)
inline int after_main(omega_ctx* c, hipStream_t waiter) {
  HIPC(c, hipEventRecord(c->ev_fork, c->stream));
  HIPC(c, hipStreamWaitEvent(waiter, c->ev_fork, 0));
  return 0;
}
inline int side_after_main(omega_ctx* c) { return after_main(c, side_stream(c)); }
// The join, `s` after everything enqueued on the side stream so far (ev_join[slot]), in its two halves: the
// back-to-back layout records early and waits behind its resolution and true-peak kernels
inline int side_join_record(omega_ctx* c, int slot) {
  HIPC(c, hipEventRecord(c->ev_join[slot], side_stream(c)));
  return 0;
}
inline int side_join_wait(omega_ctx* c, int slot, hipStream_t s) {
  HIPC(c, hipStreamWaitEvent(s, c->ev_join[slot], 0));
  return 0;
}
inline int main_after_side(omega_ctx* c, int slot) {
  if (int e = side_join_record(c, slot)) return e;
  return side_join_wait(c, slot, c->stream);
}

// ---- tables and ordering shared by several families ----
int get_window(omega_ctx* c, int m, int kind, float** out);  // capi_core.cpp
int get_rot(omega_ctx* c, int M, float2** out);              // capi_core.cpp
void drop_graphs(omega_ctx* c);                              // capi_core.cpp (the graph cache emptied)
int tr_pow2_tables(omega_ctx* c, int n, const double2** tw, const double2** tw2);  // capi_time.cpp
// capi_batch.cpp, shared with the level entry points of capi_level.cpp
int flush_meters(omega_ctx* c, hipStream_t on = nullptr);
int get_kw_tab(omega_ctx* c, int M, BiquadTab** out);
hipError_t tp_launch(int W, const SpectralParams& sp, hipStream_t s);
SpectralParams spectral_params(omega_ctx* c);
std::vector<int64_t> chunk_frames(int64_t n_frames);
std::vector<MeterPrepParams> meter_chunks(const omega_ctx* c, const std::vector<ChunkSync>& chunks, const float* lufs,
                                          const float* tp, double* out);

// capi_spectrum.cpp: omega_chroma's projection for (n_bins, df) from omega_ctx::chroma_mats, built on first use --
// the [12, hi - lo] matrix and the bin range [lo, hi) it covers
struct ChromaMat {
  const double* mat;
  int lo, hi;
};
int get_chroma_mat(omega_ctx* c, int n_bins, double df, ChromaMat* out);

// ---- host-memory staging (inline: omega_process_frames calls these on every step) ----
// Page-locked host buffer of at least `bytes` (grown on demand; hipHostMalloc).
inline int pinned_buf(omega_ctx* c, DevBuf& b, size_t bytes) {
  if (b.n >= bytes) return 0;
  if (b.p) (void)hipHostFree(b.p);
  b.p = nullptr;
  b.n = 0;
  const size_t n = std::max<size_t>(bytes, 4096);
  const hipError_t e = hipHostMalloc(&b.p, n, hipHostMallocDefault);
  if (e != hipSuccess) return fail(c, OMEGA_ENOMEM, "staging hipHostMalloc(%zu): %s", n, hipGetErrorString(e));
  b.n = n;
  return 0;
}

// staging buffer slot i of at least bytes
inline int stage_buf(omega_ctx* c, int i, size_t bytes, void** out) {
  if ((int)c->stage.size() <= i) c->stage.resize(i + 1);
  DevBuf& b = c->stage[i];
  if (b.n < bytes) {
    if (b.p) {
      // (an overlapped pipelined batch on a batch stream, or its meter segment, may still use the slot)
      for (hipStream_t f : c->bs)
        if (f) HIPC(c, hipStreamSynchronize(f));
      (void)hipFree(b.p);
    }
    b.p = nullptr;
    b.n = 0;
    const hipError_t e = hipMalloc(&b.p, std::max<size_t>(bytes, 256));
    if (e != hipSuccess) return fail(c, OMEGA_ENOMEM, "staging hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    b.n = std::max<size_t>(bytes, 256);
  }
  *out = b.p;
  return 0;
}

// Host input -> device-visible buffer: copied into the slot's page-locked buffer on the CPU. Up to
// kZeroCopyIn bytes the kernels read it there (one fabric read per element, no copy command before the
// launch); larger inputs follow with an async H2D copy into the slot's device buffer (a pageable source
// would make the runtime stage and wait on every copy).
constexpr size_t kZeroCopyIn = 256 * 1024;
constexpr size_t kZeroCopyOut = 256 * 1024;
constexpr size_t kZeroCopyTag = (size_t)1 << 62;  // HostOut::arena_off of an output in zc_pin
inline int stage_in(omega_ctx* c, int slot, const void* host, size_t bytes, const void** dev) {
  if ((int)c->pin.size() <= slot) c->pin.resize(slot + 1);
  int e = pinned_buf(c, c->pin[slot], bytes);
  if (e) return e;
  if (bytes) std::memcpy(c->pin[slot].p, host, bytes);
  if (bytes <= kZeroCopyIn) {
    void* dp = nullptr;
    HIPC(c, hipHostGetDevicePointer(&dp, c->pin[slot].p, 0));
    *dev = dp;
    return 0;
  }
  void* d = nullptr;
  e = stage_buf(c, slot, bytes, &d);
  if (e) return e;
  HIPC(c, hipMemcpyAsync(d, c->pin[slot].p, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = d;
  return 0;
}

// Host output: a device range of the call's output arena, or (zc_ok) of the zero-copy buffer, each with
// its own use counter, both reset by the call's first output. The device arena is grown, when an earlier
// call wanted more, at this call's first output placed in it (nothing of this call is in it yet); this
// call's outputs past its end use their own slots. finish_host copies the arena back in one D2H copy.
template <class T>
int stage_out(omega_ctx* c, int slot, T* host, size_t count, std::vector<HostOut>& outs, T** dev) {
  if (!host) {
    *dev = nullptr;
    return 0;
  }
  if (outs.empty()) {
    c->oarena_used = 0;
    c->zc_used = 0;
  }
  const size_t bytes = count * sizeof(T);
  if (c->zc_ok) {
    // small outputs of a store-only call: straight into page-locked memory (no copy command after the
    // kernels; finish_host only copies them to the caller's buffers on the CPU)
    const size_t off = (c->zc_used + 255) & ~(size_t)255;
    if (off + bytes <= kZeroCopyOut) {
      if (!c->zc_pin.p) {
        if (int e = pinned_buf(c, c->zc_pin, kZeroCopyOut)) return e;
        HIPC(c, hipHostGetDevicePointer(&c->zc_dev, c->zc_pin.p, 0));
      }
      c->zc_used = off + bytes;
      outs.push_back({host, static_cast<char*>(c->zc_pin.p) + off, bytes, kZeroCopyTag + off});
      *dev = reinterpret_cast<T*>(static_cast<char*>(c->zc_dev) + off);
      return 0;
    }
  }
  if (c->oarena_used == 0) {
    if (c->oarena_want > c->oarena.n) {
      const size_t n = c->oarena_want + c->oarena_want / 4;
      if (c->oarena.p) (void)hipFree(c->oarena.p);
      c->oarena.p = nullptr;
      c->oarena.n = 0;
      if (hipMalloc(&c->oarena.p, n) == hipSuccess) {
        c->oarena.n = n;
        if (int e = pinned_buf(c, c->oarena_pin, n)) return e;
      }
    }
  }
  const size_t off = (c->oarena_used + 255) & ~(size_t)255;
  if (off + bytes <= c->oarena.n && c->oarena_pin.n >= c->oarena.n) {
    c->oarena_used = off + bytes;
    outs.push_back({host, static_cast<char*>(c->oarena.p) + off, bytes, off});
    *dev = reinterpret_cast<T*>(static_cast<char*>(c->oarena.p) + off);
    return 0;
  }
  c->oarena_want = std::max(c->oarena_want, off + bytes);
  void* d = nullptr;
  int e = stage_buf(c, slot, bytes, &d);
  if (e) return e;
  outs.push_back({host, d, bytes, ~(size_t)0});
  *dev = static_cast<T*>(d);
  return 0;
}

// A device-side ordering wait that expired (meters.hip: the prep kernel's wait for the batch's
// K-weighting count, the join of the LUFS meters into the caller's stream) means some meter aggregates
// were computed from, or returned before, incomplete inputs: report it once as OMEGA_EHIP.
inline int check_device_err(omega_ctx* c) {
  if (!c->h_err) return 0;
  volatile unsigned* e = c->h_err;
  const unsigned prep = e[0], join = e[1];
  if (!prep && !join) return 0;
  e[0] = 0;
  e[1] = 0;
  return fail(c, OMEGA_EHIP, "device-side meter ordering wait expired (%s%s%s): meter aggregates of an earlier call "
              "may be stale", prep ? "meter prep waiting for the K-weighting count" : "", prep && join ? ", " : "",
              join ? "caller's stream joining the LUFS meters" : "");
}

// Host-memory calls: copy the outputs back and wait; an ordering wait of THIS call that expired is
// reported by this call (device-memory calls report it at the next call or omega_synchronize).
inline int finish_host(omega_ctx* c, const std::vector<HostOut>& outs) {
  c->zc_ok = false;
  size_t span = 0;
  for (const HostOut& o : outs) {
    if (o.arena_off == ~(size_t)0)
      HIPC(c, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream));
    else if (o.arena_off < kZeroCopyTag)
      span = std::max(span, o.arena_off + o.bytes);
  }
  if (span) HIPC(c, hipMemcpyAsync(c->oarena_pin.p, c->oarena.p, span, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (c->fork[0] && hipStreamQuery(c->fork[0]) != hipSuccess) HIPC(c, hipStreamSynchronize(c->fork[0]));
  for (const HostOut& o : outs) {
    if (o.arena_off == ~(size_t)0) continue;
    const char* src = o.arena_off >= kZeroCopyTag ? static_cast<const char*>(o.dev)
                                                   : static_cast<char*>(c->oarena_pin.p) + o.arena_off;
    std::memcpy(o.host, src, o.bytes);
  }
  return check_device_err(c);
}

// One entry point's staging. in() / out() give the pointer the kernels use: the caller's own for
// OMEGA_MEM_DEVICE (and for a null pointer), else the staged one of stage_in / stage_out. Slots go in
// call order, from `slot` on where one is given. The first error stays in `err` and nothing more is
// staged; finish() copies the outputs back and waits (finish_host).
struct HostCall {
  omega_ctx* c;
  const bool host;
  int next = 0, err = 0;
  std::vector<HostOut> outs;
  HostCall(omega_ctx* ctx, int mem) : c(ctx), host(mem == OMEGA_MEM_HOST) {}
  template <class T>
  const T* in(const T* p, size_t bytes, int slot = -1) {
    if (slot >= 0) next = slot;
    const int s = next++;
    if (!host || !p) return p;
    if (err) return nullptr;
    const void* d = nullptr;
    err = stage_in(c, s, p, bytes, &d);
    return static_cast<const T*>(d);
  }
  template <class T>
  T* out(T* p, size_t count, int slot = -1) {
    if (slot >= 0) next = slot;
    const int s = next++;
    if (!host) return p;
    if (err) return nullptr;
    T* d = nullptr;
    err = stage_out(c, s, p, count, outs, &d);
    return d;
  }
  // A batch of n_frames rows of `width` elements staged like in(): exactly the span the batch touches
  Rows rows(const void* p, int64_t stride, int64_t width, int f64, int64_t n_frames) {
    Rows r{nullptr, stride, f64 ? 1 : 0};
    r.base = in(p, r.span_bytes(n_frames, width));
    return r;
  }
  Rows32 rows32(const float* p, int64_t stride, int64_t width, int64_t n_frames) {
    Rows32 r{nullptr, stride};
    r.base = in(p, r.span_bytes(n_frames, width));
    return r;
  }
  int finish() { return host ? finish_host(c, outs) : 0; }
};

// [lo, lo + n): the i < K whose frequency passes pred, one range over an increasing table (none: lo = 0)
template <class F, class P>
void mask_range(int K, F freq_at, P pred, int* lo, int* n) {
  *lo = 0;
  *n = 0;
  for (int i = 0; i < K; ++i)
    if (pred(freq_at(i))) {
      if (!*n) *lo = i;
      ++*n;
    }
}

// body(f0, count) over [0, n_frames) in launches of at most `per` frames; stops at the first error
template <class F>
int for_frame_chunks(int64_t n_frames, int64_t per, F body) {
  for (int64_t f0 = 0; f0 < n_frames; f0 += per)
    if (int e = body(f0, std::min(per, n_frames - f0))) return e;
  return 0;
}

// A call of no frames: the caller's state passes through (a stream's first call: zeros)
inline int pass_state_through(omega_ctx* c, const double* sin, double* sout, size_t bytes) {
  if (!sout || sout == sin) return 0;
  if (sin)
    HIPC(c, hipMemcpyAsync(sout, sin, bytes, hipMemcpyDefault, c->stream));
  else
    HIPC(c, hipMemsetAsync(sout, 0, bytes, c->stream));
  return 0;
}

// for_frame_chunks for a family whose launches carry a state of state_len doubles from `sin` to `sout` (either
// may be null): body(f0, count, state_in, state_out) per launch, chained as frames.hpp's chain_chunks plans
// through the context's two blobs (allocated here on first use, blob_len doubles each)
template <class F>
int chained_frame_chunks(omega_ctx* c, double* (&blob)[2], size_t blob_len, size_t state_len, int64_t n_frames,
                         int64_t per, const double* sin, double* sout, F body) {
  for (double*& b : blob)
    if (!b)
      if (int e = dalloc(c, &b, blob_len)) return e;
  auto at = [&](ChainBuf b) { return b == kChainOut ? sout : (b == kChainNone ? nullptr : blob[b]); };
  auto launch = [&](int64_t f0, int64_t count, ChainBuf read, ChainStep s) -> int {
    double* w = at(s.write);
    if (int e = body(f0, count, read == kChainIn ? sin : at(read), w)) return e;
    if (s.copy_back) HIPC(c, hipMemcpyAsync(sout, w, state_len * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return 0;
  };
  return chain_chunks(n_frames, per, sout != nullptr, sout == sin, launch);
}

}  // namespace omega_host

// the any-length transform's plan and launches on `s` (capi_level.cpp), shared by omega_true_peak_os and omega_rfft
extern "C" {
int get_any_plan(omega_ctx* c, int N, omega_ctx::AnyPlan** out);
int run_any(omega_ctx* c, AnyFftParams p, int truepeak, hipStream_t s);
}
