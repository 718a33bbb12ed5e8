"""ctypes binding of libomega.so (include/omega.h). No torch types cross this boundary: plain
pointers and sizes. The library is loaded from the package's in-tree ``lib/`` and the import fails
loudly when it is missing -- there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libomega.so")

MAX_RES = 4
N_METERS = 5
MEM_HOST, MEM_DEVICE = 0, 1
WIN = {"blackman": 0, "hann": 1, "hamming": 2, "rect": 3}
BANDS_MAX, BANDS_MEAN = 0, 1
WEIGHT = {"K": 0, "A": 1, "C": 2, "Z": 3}
OK, EINVAL, EHIP, ENOMEM, EUNSUP = 0, -1, -2, -3, -4


class Resolution(C.Structure):
    _fields_ = [("freq_lo", C.c_double), ("freq_hi", C.c_double), ("fft_size", C.c_int32),
                ("hop_size", C.c_int32), ("weight", C.c_double), ("window", C.c_int32)]


class Config(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("max_freq", C.c_double), ("n_res", C.c_int32),
                ("res", Resolution * MAX_RES), ("apply_weighting", C.c_int32), ("target_bins", C.c_int32),
                ("frame_size", C.c_int32), ("n_channels", C.c_int32), ("gate_lufs", C.c_double),
                ("momentary_len", C.c_int32), ("short_len", C.c_int32), ("integrated_len", C.c_int32),
                ("peak_len", C.c_int32)]


class Outputs(C.Structure):
    _fields_ = [("combined", C.c_void_p), ("lufs_inst", C.c_void_p), ("true_peak_db", C.c_void_p),
                ("meters", C.c_void_p), ("mag", C.c_void_p * MAX_RES), ("weighted", C.c_void_p)]


class IngestConfig(C.Structure):
    _fields_ = [("format", C.c_int32), ("sample_rate", C.c_int32), ("hop", C.c_int32), ("batch_hops", C.c_int32),
                ("ring_slots", C.c_int32), ("max_pending_batches", C.c_int32), ("chunk_size", C.c_int32), ("gain", C.c_float), ("gate", C.c_int32),
                ("noise_floor", C.c_double), ("silence_threshold_seconds", C.c_double),
                ("background_alpha", C.c_double), ("want", C.c_int32)]


class IngestStats(C.Structure):
    _fields_ = [("bytes_in", C.c_int64), ("batches", C.c_int64), ("frames", C.c_int64),
                ("frames_polled", C.c_int64), ("dropped_frames", C.c_int64)]


class PitchConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("min_pitch", C.c_double), ("max_pitch", C.c_double),
                ("yin_threshold", C.c_double), ("yin_window_size", C.c_int32), ("enable_preprocessing", C.c_int32),
                ("highpass_frequency", C.c_double), ("highpass_order", C.c_int32), ("enable_compression", C.c_int32),
                ("compression_threshold", C.c_double), ("compression_ratio", C.c_double)]


class HarmonicConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_bins", C.c_int32), ("max_series", C.c_int32)]


class GenreConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_bins", C.c_int32)]


class HipHopConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_bins", C.c_int32)]


class PhaseConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("m", C.c_int32)]


class RoomConfig(C.Structure):
    _fields_ = [(k, C.c_double) for k in (
        "sample_rate", "min_frequency", "max_frequency", "peak_threshold_multiplier", "minimum_prominence_std",
        "min_q_factor", "max_q_factor", "minimum_severity")]


class VoiceConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("n_bins", C.c_int32), ("frame_len", C.c_int32)]


class TdetectConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("n_bins", C.c_int32), ("frame_len", C.c_int32)]


class BassZoomConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("frame_len", C.c_int32)]


class RhythmConfig(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("frame_len", C.c_int32)]


class WaterfallConfig(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("first_bin", C.c_int32), ("n_cells", C.c_int32)]


class TonalConfig(C.Structure):
    _fields_ = [("genre", C.c_int32)]


class MeterPanelConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("frame_len", C.c_int32), ("level_len", C.c_int32),
                ("peak_len", C.c_int32), ("range_len", C.c_int32), ("n_bins", C.c_int32), ("hist_lo", C.c_double),
                ("hist_hi", C.c_double)]


FMT = {"float32le": 0, "s16le": 1}
INGEST_COMBINED, INGEST_LUFS, INGEST_TRUE_PEAK, INGEST_METERS = 1, 2, 4, 8


class OmegaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libomega error {code}: {msg}")
        self.code = code


class UnsupportedError(OmegaError):
    """A valid reference call this build does not cover (e.g. a non power-of-two frame)."""


EXPORTS = {
    "omega_version": (C.c_char_p, []),
    "omega_config_default": (None, [C.POINTER(Config)]),
    "omega_create": (C.c_int, [C.POINTER(Config), C.c_int, C.POINTER(C.c_void_p)]),
    "omega_destroy": (None, [C.c_void_p]),
    "omega_last_error": (C.c_char_p, [C.c_void_p]),
    "omega_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "omega_check_queues": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "omega_synchronize": (C.c_int, [C.c_void_p]),
    "omega_set_meter_pipelining": (C.c_int, [C.c_void_p, C.c_int]),
    "omega_flush_meters": (C.c_int, [C.c_void_p]),
    "omega_get_stream": (C.c_void_p, [C.c_void_p]),
    "omega_get_config": (C.c_int, [C.c_void_p, C.POINTER(Config), C.POINTER(C.c_int)]),
    "omega_vu_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_int]),
    "omega_vu_reset": (C.c_int, [C.c_void_p]),
    "omega_transients": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                   C.c_int]),
    "omega_pitch_config_default": (None, [C.POINTER(PitchConfig)]),
    "omega_pitch_configure": (C.c_int, [C.c_void_p, C.POINTER(PitchConfig)]),
    "omega_pitch_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                     C.c_int]),
    "omega_harmonic_config_default": (None, [C.POINTER(HarmonicConfig)]),
    "omega_harmonic_configure": (C.c_int, [C.c_void_p, C.POINTER(HarmonicConfig), C.c_void_p]),
    "omega_harmonic_analyze": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "omega_harmonic_reset": (C.c_int, [C.c_void_p]),
    "omega_harmonic_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_double, C.c_void_p, C.c_int]),
    "omega_genre_config_default": (None, [C.POINTER(GenreConfig)]),
    "omega_genre_configure": (C.c_int, [C.c_void_p, C.POINTER(GenreConfig), C.c_void_p]),
    "omega_genre_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                       C.c_int64, C.c_void_p, C.c_void_p, C.c_int]),
    "omega_genre_reset": (C.c_int, [C.c_void_p]),
    "omega_hiphop_config_default": (None, [C.POINTER(HipHopConfig)]),
    "omega_hiphop_configure": (C.c_int, [C.c_void_p, C.POINTER(HipHopConfig), C.c_void_p]),
    "omega_hiphop_get_sos": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "omega_hiphop_design_sos": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p]),
    "omega_hiphop_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                        C.c_int64, C.c_void_p, C.c_void_p, C.c_int]),
    "omega_phase_config_default": (None, [C.POINTER(PhaseConfig)]),
    "omega_phase_band_ranges": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "omega_phase_hanning": (C.c_int, [C.c_int32, C.c_void_p]),
    "omega_phase_configure": (C.c_int, [C.c_void_p, C.POINTER(PhaseConfig), C.c_void_p]),
    "omega_phase_correlation": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_int]),
    "omega_room_config_default": (None, [C.POINTER(RoomConfig)]),
    "omega_room_bin_range": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p]),
    "omega_room_configure": (C.c_int, [C.c_void_p, C.POINTER(RoomConfig), C.c_void_p, C.c_int32, C.c_void_p]),
    "omega_room_modes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int]),
    "omega_room_decay": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_int]),
    "omega_voice_config_default": (None, [C.POINTER(VoiceConfig)]),
    "omega_voice_bin_range": (C.c_int, [C.c_double, C.c_int32, C.c_void_p]),
    "omega_voice_configure": (C.c_int, [C.c_void_p, C.POINTER(VoiceConfig)]),
    "omega_voice_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                       C.c_int64, C.c_void_p, C.c_int]),
    "omega_tdetect_config_default": (None, [C.POINTER(TdetectConfig)]),
    "omega_tdetect_band_indices": (C.c_int, [C.c_double, C.c_int32, C.c_void_p]),
    "omega_tdetect_configure": (C.c_int, [C.c_void_p, C.POINTER(TdetectConfig)]),
    "omega_tdetect_state_size": (C.c_int64, []),
    "omega_tdetect_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "omega_basszoom_config_default": (None, [C.POINTER(BassZoomConfig)]),
    "omega_basszoom_mapping": (C.c_int, [C.c_double] + [C.c_void_p] * 6),
    "omega_basszoom_configure": (C.c_int, [C.c_void_p, C.POINTER(BassZoomConfig)]),
    "omega_basszoom_state_size": (C.c_int64, []),
    "omega_basszoom_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64]
                                + [C.c_void_p] * 6 + [C.c_int]),
    "omega_rhythm_config_default": (None, [C.POINTER(RhythmConfig)]),
    "omega_rhythm_configure": (C.c_int, [C.c_void_p, C.POINTER(RhythmConfig), C.c_void_p, C.c_void_p]),
    "omega_rhythm_state_size": (C.c_int64, [C.c_int32]),
    "omega_rhythm_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                        C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "omega_waterfall_config_default": (None, [C.POINTER(WaterfallConfig)]),
    "omega_waterfall_mapping": (C.c_int, [C.c_double, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "omega_waterfall_configure": (C.c_int, [C.c_void_p, C.POINTER(WaterfallConfig)]),
    "omega_waterfall_state_size": (C.c_int64, []),
    "omega_waterfall_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_double,
                                       C.c_int32] + [C.c_void_p] * 5 + [C.c_int]),
    "omega_waterfall_colors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_int]),
    "omega_tonal_config_default": (None, [C.POINTER(TonalConfig)]),
    "omega_tonal_configure": (C.c_int, [C.c_void_p, C.POINTER(TonalConfig)]),
    "omega_tonal_state_size": (C.c_int64, []),
    "omega_tonal_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 9 + [C.c_int]),
    "omega_tonal_spectra": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double] + [C.c_void_p] * 9
                            + [C.c_int]),
    "omega_meterpanel_config_default": (None, [C.POINTER(MeterPanelConfig)]),
    "omega_meterpanel_state_size": (C.c_int64, [C.POINTER(MeterPanelConfig)]),
    "omega_meterpanel_edges": (C.c_int, [C.POINTER(MeterPanelConfig), C.c_void_p]),
    "omega_meterpanel_unpack": (C.c_int, [C.POINTER(MeterPanelConfig)] + [C.c_void_p] * 9),
    "omega_meterpanel_configure": (C.c_int, [C.c_void_p, C.POINTER(MeterPanelConfig)]),
    "omega_meterpanel_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                          C.c_int64, C.c_int32] + [C.c_void_p] * 4 + [C.c_int]),
    "omega_ingest_config_default": (None, [C.POINTER(IngestConfig)]),
    "omega_ingest_create": (C.c_int, [C.c_void_p, C.POINTER(IngestConfig), C.POINTER(C.c_void_p)]),
    "omega_ingest_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "omega_ingest_flush": (C.c_int, [C.c_void_p]),
    "omega_ingest_poll": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Outputs), C.c_int, C.POINTER(C.c_int64)]),
    "omega_ingest_get_stats": (C.c_int, [C.c_void_p, C.POINTER(IngestStats)]),
    "omega_ingest_last_error": (C.c_char_p, [C.c_void_p]),
    "omega_ingest_destroy": (None, [C.c_void_p]),
    "omega_set_graphs": (C.c_int, [C.c_void_p, C.c_int]),
    "omega_process_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                       C.POINTER(Outputs), C.c_int]),
    "omega_process_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                       C.POINTER(Outputs), C.c_int, C.POINTER(C.c_int64)]),
    "omega_spectra": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int]),
    "omega_combine": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int64, C.c_void_p, C.c_int]),
    "omega_true_peak": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int]),
    "omega_true_peak_os": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int]),
    "omega_k_weighting": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_int]),
    "omega_weighting": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_int]),
    "omega_meter_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]),
    "omega_meter_reset": (C.c_int, [C.c_void_p]),
    "omega_meter_load_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int]),
    "omega_calculate_lufs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "omega_bands_create": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "omega_bands_destroy": (None, [C.c_void_p]),
    "omega_bands_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                    C.c_int]),
    "omega_chroma": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_int]),
    "omega_drum_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_double,
                                      C.c_void_p, C.c_int]),
    "omega_drum_reset": (C.c_int, [C.c_void_p]),
    "omega_post_configure": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_float]
                             + [C.c_void_p] * 3 + [C.c_int32]),
    "omega_post_process": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "omega_post_reset": (C.c_int, [C.c_void_p]),
    "omega_rfft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                             C.c_int]),
}

_lib = None


def _share_torch_hip_runtime() -> None:
    """One HIP runtime per process. torch-ROCm ships its own libamdhip64 (SONAME libamdhip64.so.7,
    like /opt/rocm's). If libomega loaded first it would bind /opt/rocm's copy and torch would then
    load a second runtime (torch reports "No HIP GPUs are available", and torch streams/events would
    not order libomega's kernels). Preloading torch's copy by path, without importing torch, makes
    libomega's NEEDED libamdhip64.so.7 resolve to the runtime torch uses."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    for d in spec.submodule_search_locations:
        p = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)
            return


def use_development_library(name: str) -> None:
    """Kernel-development tools only (tools/stamps.py, tools/wgtrace.py): load lib/<name> (e.g.
    libomega_dev.so from `make dev`) instead of libomega.so. Must run before the first lib() call; the
    product path never calls it and reads no environment variable to pick its library."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("libomega is already loaded")
    LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", name)


def lib() -> C.CDLL:
    """Load libomega.so once (raises if the HIP library was not built: no fallback)."""
    global _lib
    if _lib is None:
        _share_torch_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libomega.so not found at {LIB_PATH}; run `make -C audio-analyzer-omega_amd` "
                              "(or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        dev = os.path.basename(LIB_PATH) != "libomega.so"
        for name, (res, args) in EXPORTS.items():
            if dev and not hasattr(L, name):  # (an older build in an A/B: its ABI's entry points only)
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(ctx, code: int) -> None:
    if code != OK:
        msg = lib().omega_last_error(ctx).decode() if ctx else ""
        raise (UnsupportedError if code == EUNSUP else OmegaError)(code, msg)


def check_plain(code: int, msg: str) -> None:
    """check() for the entry points that take no context and so leave no error text: msg says what a
    refusal means."""
    if code != OK:
        raise OmegaError(code, msg)
