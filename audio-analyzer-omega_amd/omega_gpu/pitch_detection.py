"""CepstralAnalyzer on the MI355X: detect_pitch_advanced
(omega4/panels/pitch_detection.py:21-611) -- cepstrum, FFT autocorrelation and YIN per frame, combined
by confidence -- over libomega.so's omega_pitch_detect, with the reference's configuration surface
(omega4/panels/pitch_detection_config.py:13-245; config file persistence is not carried over).

``detect_batch(frames)`` analyses a batch of one stream's frames in one launch and advances the
histories in order; ``detect_pitch_advanced(_safe)(signal)`` return the reference's dicts. The note
name, the stability score and the two histories (:435-483) are scalar float64 work on the host. Device
batches follow the facades' common row rule (_marshal.rows): overlapping rows are read in place; a batch
with ``stride(0) < 1`` and F > 1 (an ``expand`` of one frame) is copied and analysed, where this facade once
left it to the library to refuse; samples that are neither float32 nor float64 become float64.

The combination follows the reference, not the configuration: the acceptance thresholds 0.15 / 0.2 /
0.25 and the weights 0.8 / 0.9 / 1.1 are hard-coded in combine_pitch_estimates (:384-393), and the
config's ``cepstral_weight`` / ``autocorr_weight`` / ``yin_weight`` / ``min_confidence_threshold``
(like its cepstral_* and autocorr_* peak fields) are carried but never read -- exactly as there.
There is no CPU fallback: a frame length the library does not build (anything but 2048, 4096 or 8192
samples at or above ``yin_window_size``) gives the default dict with ``error`` set.
"""
from __future__ import annotations

import ctypes as C
import logging
import time
from collections import deque
from dataclasses import asdict, dataclass, fields
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

logger = logging.getLogger(__name__)
COLUMNS = ("pitch", "confidence", "cepstral_pitch", "cepstral_confidence", "autocorr_pitch", "autocorr_confidence",
           "yin_pitch", "yin_confidence", "rms", "flags")
FLAG_NONFINITE, FLAG_SILENT = 1, 2
NOTE_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")


@dataclass
class PitchDetectionConfig:
    """The reference's configuration fields and defaults (pitch_detection_config.py:13-72)."""
    sample_rate: int = 48000
    min_pitch: float = 50.0
    max_pitch: float = 2000.0
    yin_threshold: float = 0.15
    yin_window_size: int = 1024
    yin_use_vectorization: bool = True
    cepstral_window_size: int = 2048
    cepstral_peak_threshold: float = 0.3
    cepstral_min_peak_distance: int = 20
    autocorr_min_correlation: float = 0.3
    autocorr_peak_distance: int = 20
    cepstral_weight: float = 0.8
    autocorr_weight: float = 0.9
    yin_weight: float = 1.1
    min_confidence_threshold: float = 0.15
    high_confidence_threshold: float = 0.8
    medium_confidence_threshold: float = 0.5
    enable_preprocessing: bool = True
    highpass_frequency: float = 80.0
    highpass_order: int = 4
    enable_compression: bool = True
    compression_threshold: float = 0.1
    compression_ratio: float = 0.5
    use_memory_pool: bool = True
    max_history_length: int = 100
    enable_threading: bool = False
    cache_filter_coefficients: bool = True
    pitch_stability_window: int = 20
    pitch_stability_threshold: float = 0.1
    enable_pitch_smoothing: bool = True
    smoothing_factor: float = 0.2
    enable_performance_monitoring: bool = False
    enable_debug_logging: bool = False
    log_processing_times: bool = False
    profile_name: str = "balanced"

    def __post_init__(self):
        self.validate()
        self.adjust_for_sample_rate()

    def validate(self) -> None:
        """:79-102 (AssertionError, like the reference)."""
        assert self.sample_rate > 0, "Sample rate must be positive"
        assert self.min_pitch > 0, "Minimum pitch must be positive"
        assert self.max_pitch > self.min_pitch, "Maximum pitch must be greater than minimum"
        assert 0 < self.yin_threshold < 1, "YIN threshold must be between 0 and 1"
        assert self.yin_window_size > 0, "YIN window size must be positive"
        assert min(self.cepstral_weight, self.autocorr_weight, self.yin_weight) >= 0, "Method weights must be non-negative"
        assert (0 <= self.min_confidence_threshold < self.medium_confidence_threshold
                < self.high_confidence_threshold <= 1), "Confidence thresholds must be properly ordered between 0 and 1"
        if self.enable_preprocessing:
            assert self.highpass_frequency > 0, "Highpass frequency must be positive"
            assert self.highpass_order > 0, "Filter order must be positive"
            assert self.highpass_frequency < self.sample_rate / 2, "Highpass frequency must be below Nyquist"

    def adjust_for_sample_rate(self) -> None:
        """:104-121: windows scaled from 48 kHz, clamped, and at least two longest periods long."""
        if self.sample_rate != 48000:
            k = self.sample_rate / 48000
            self.yin_window_size = int(self.yin_window_size * k)
            self.cepstral_window_size = int(self.cepstral_window_size * k)
        self.yin_window_size = max(512, min(4096, self.yin_window_size))
        self.cepstral_window_size = max(1024, min(8192, self.cepstral_window_size))
        longest = int(self.sample_rate / self.min_pitch)
        self.yin_window_size = max(self.yin_window_size, 2 * longest)
        self.cepstral_window_size = max(self.cepstral_window_size, 2 * longest)

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)

    def update_from_dict(self, updates: Dict[str, Any]) -> None:
        names = {f.name for f in fields(self)}
        for k, v in updates.items():
            if k in names:
                setattr(self, k, v)
        self.validate()
        self.adjust_for_sample_rate()


# what each reference preset sets beside the defaults (pitch_detection_config.py:177-233)
_PRESETS: Dict[str, Dict[str, Any]] = {
    "low_latency": dict(yin_window_size=512, cepstral_window_size=1024, enable_preprocessing=False,
                        enable_pitch_smoothing=False),
    "high_accuracy": dict(yin_window_size=2048, cepstral_window_size=4096, yin_threshold=0.1, smoothing_factor=0.3,
                          high_confidence_threshold=0.85, min_confidence_threshold=0.2),
    "balanced": {},
    "voice_optimized": dict(min_pitch=80.0, max_pitch=1000.0, highpass_frequency=70.0, compression_threshold=0.08,
                            yin_weight=1.2, cepstral_weight=0.9, autocorr_weight=0.7),
    "music_optimized": dict(min_pitch=40.0, max_pitch=4000.0, highpass_frequency=30.0, compression_threshold=0.15,
                            cepstral_weight=1.0, autocorr_weight=1.0, yin_weight=1.0, min_confidence_threshold=0.25),
}
PRESET_CONFIGS = {name: PitchDetectionConfig(profile_name=name, **kw) for name, kw in _PRESETS.items()}


def get_preset_config(preset_name: str) -> PitchDetectionConfig:
    if preset_name not in PRESET_CONFIGS:
        raise ValueError(f"Unknown preset: {preset_name}. Available: {list(PRESET_CONFIGS.keys())}")
    return PRESET_CONFIGS[preset_name]


def list_presets() -> List[str]:
    return list(PRESET_CONFIGS.keys())


class CepstralAnalyzer:
    def __init__(self, sample_rate: int = 48000, config: Optional[PitchDetectionConfig] = None, device: int = 0):
        self.sample_rate = sample_rate
        self.config = config or PitchDetectionConfig(sample_rate=sample_rate)
        self.min_pitch, self.max_pitch = self.config.min_pitch, self.config.max_pitch
        self.min_period = int(sample_rate / self.max_pitch)
        self.max_period = int(sample_rate / self.min_pitch)
        self.yin_threshold = self.config.yin_threshold
        self.yin_window_size = self.config.yin_window_size
        self.high_confidence = self.config.high_confidence_threshold
        self.medium_confidence = self.config.medium_confidence_threshold
        self.pitch_history = deque(maxlen=self.config.max_history_length)
        self.confidence_history = deque(maxlen=self.config.max_history_length)
        self.processing_times = deque(maxlen=100) if self.config.enable_performance_monitoring else None
        self.error_count = 0
        self.last_error_time = 0
        self._eng = utility_engine(sample_rate, device)
        c = self.config
        cfg = L.PitchConfig(int(sample_rate), float(c.min_pitch), float(c.max_pitch), float(c.yin_threshold),
                            int(c.yin_window_size), int(bool(c.enable_preprocessing)), float(c.highpass_frequency),
                            int(c.highpass_order), int(bool(c.enable_compression)), float(c.compression_threshold),
                            float(c.compression_ratio))
        self._eng._check(L.lib().omega_pitch_configure(self._eng._ctx, C.byref(cfg)))

    # -- the device part --
    def _detect(self, frames):
        """frames [F, n] -> ([F, 10] host float64, the block as returned to detect_batch's caller)."""
        frames, frame_ptr, stride, f64 = M.rows(frames, _is_torch(frames), "frames must be [F, n]", audio=True)
        F, n = frames.shape
        out = M.alloc(frames, (F, len(COLUMNS)), np.float64)
        M.call(self._eng, L.lib().omega_pitch_detect, frames, frame_ptr, f64, F, n, stride, _ptr(out))
        return (out.cpu().numpy() if _is_torch(out) else out), out

    def detect_batch(self, frames):
        """frames [F, n] (float32 / float64; host numpy, or device torch -- rows may overlap, e.g. an
        ``unfold`` view of a stream) -> [F, 10] float64 in COLUMNS order (numpy for host input, a device
        tensor for device input). Flagged frames (non-finite, silent) are zero rows and, like frames shorter
        than yin_window_size, leave the histories alone, as the reference's early returns do."""
        host, out = self._detect(frames)
        if host.shape[0] and frames.shape[1] >= self.yin_window_size:
            for row in host:
                if row[9] == 0:
                    self.pitch_history.append(float(row[0]))
                    self.confidence_history.append(float(row[1]))
        return out

    # -- the reference's surface --
    def validate_audio_input(self, signal) -> Tuple[bool, str]:
        """:64-93, with the level and the finiteness test on the host for this one frame."""
        if signal is None:
            return False, "Signal is None"
        if not isinstance(signal, np.ndarray):
            return False, f"Signal must be numpy array, got {type(signal)}"
        if len(signal) == 0:
            return False, "Signal is empty"
        if not np.isfinite(signal).all():
            return False, "Signal contains non-finite values (inf/nan)"
        if signal.dtype not in [np.float32, np.float64]:
            return False, f"Signal must be float32 or float64, got {signal.dtype}"
        if len(signal) < self.min_period * 2:
            return False, f"Signal too short for pitch detection (need at least {self.min_period * 2} samples)"
        if np.sqrt(np.mean(signal ** 2)) < 1e-6:
            return False, "Signal level too low (essentially silence)"
        return True, ""

    def pitch_to_note(self, pitch: float) -> Tuple[str, int, int]:
        """:435-456"""
        if pitch <= 0:
            return "", 0, 0
        c0 = 440.0 * (2 ** (-4.75))
        semitones = 12 * np.log2(pitch / c0)
        nearest = int(round(semitones))
        return NOTE_NAMES[nearest % 12], nearest // 12, int((semitones - nearest) * 100)

    def calculate_pitch_stability(self) -> float:
        """:458-483"""
        if len(self.pitch_history) < 10:
            return 0.0
        pitches, confs = list(self.pitch_history)[-20:], list(self.confidence_history)[-20:]
        valid = [p for p, c in zip(pitches, confs) if c > 0.3 and p > 0]
        if len(valid) < 5:
            return 0.0
        mean = np.mean(valid)
        return max(0.0, 1.0 - np.std(valid) / mean * 10) if mean > 0 else 0.0

    @staticmethod
    def _zero_result() -> Dict[str, Any]:
        return {"pitch": 0.0, "confidence": 0.0, "note": "", "cents_offset": 0, "octave": 0, "stability": 0.0}

    def detect_pitch_advanced(self, signal) -> Dict[str, Any]:
        """:485-556 for one frame. Raises UnsupportedError for a frame length the library does not build."""
        if len(signal) < self.yin_window_size:
            return self._zero_result()
        row = self._detect(np.asarray(signal)[None, :])[0][0]
        flags = int(row[9])
        if flags & FLAG_NONFINITE:
            raise ValueError("Signal contains non-finite values (inf/nan)")
        if flags & FLAG_SILENT:
            raise ValueError("Signal level too low (essentially silence)")
        pitch, confidence = float(row[0]), float(row[1])

        def pair(p, c, f32=False):
            if p == 0.0 and c == 0.0:
                return 0.0, 0.0
            return np.float64(p), (np.float32(c) if f32 else np.float64(c))
        methods = {"cepstral": pair(row[2], row[3]), "autocorr": pair(row[4], row[5], True), "yin": pair(row[6], row[7])}
        self.pitch_history.append(pitch)
        self.confidence_history.append(confidence)
        note, octave, cents = self.pitch_to_note(pitch)
        return {"pitch": pitch, "confidence": confidence, "note": note, "octave": octave, "cents_offset": cents,
                "stability": self.calculate_pitch_stability(), "methods": methods}

    def detect_pitch_advanced_safe(self, signal) -> Dict[str, Any]:
        """:558-611: validation, then detect_pitch_advanced; whatever goes wrong is logged (at most once a
        second) and reported in the default dict's ``error``."""
        start = time.time() if self.config.enable_performance_monitoring else None
        default = {"pitch": 0.0, "confidence": 0.0, "note": "", "octave": 0, "cents_offset": 0, "stability": 0.0,
                   "methods": {}, "error": None}
        try:
            ok, msg = self.validate_audio_input(signal)
            if not ok:
                logger.debug("Invalid audio input: %s", msg)
                default["error"] = msg
                return default
            result = self.detect_pitch_advanced(signal)
            if start is not None:
                self.processing_times.append((time.time() - start) * 1000)
            return result
        except Exception as e:
            now = time.time()
            if now - self.last_error_time > 1.0:
                logger.error("Pitch detection error: %s", e)
                self.last_error_time = now
            self.error_count += 1
            default["error"] = str(e)
            return default

    def get_performance_stats(self) -> Dict[str, float]:
        if not self.config.enable_performance_monitoring or not self.processing_times:
            return {}
        t = list(self.processing_times)
        return {"avg_time_ms": np.mean(t), "max_time_ms": np.max(t), "min_time_ms": np.min(t), "std_time_ms": np.std(t),
                "error_count": self.error_count}
