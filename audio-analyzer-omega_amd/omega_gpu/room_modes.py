"""Room acoustics on the MI355X: RoomModeAnalyzer
(omega4/analyzers/room_modes.py:19-499, room_mode_config.py:9-74) over libomega.so's omega_room_modes and
omega_room_decay.

    rm = RoomModeAnalyzer(48000)
    modes = rm.detect_room_modes(spectrum, freqs)        # [{'frequency', 'magnitude', 'q_factor', ...}, ...]
    per_frame = rm.detect_room_modes_batch(spectra, freqs)   # [F, n_bins] -> F lists
    rm.update_audio_history(chunk); rm.calculate_rt60_estimate("schroeder")

The device computes, per spectrum and in one workgroup: mean and std of the in-range bins, scipy's
find_peaks(height=, prominence=) peak set, and per peak the Q factor, severity, type and bandwidth, ordered
like the reference's stable sort; and per sample history the Schroeder curve's -5 / -10 / -35 dB crossings,
the least-squares decay line with its r_squared, and the frames' energies (include/omega.h has the columns).
The scalar ends stay on the host: the dicts and type strings, the RT60 clamps and confidences, the `simple`
method's fit over the 30-60 frame energies, classify_room_mode, get_speed_of_sound, estimate_room_dimensions
and the history deque.

Departures, both deliberate. (1) Everything is float64 whatever the input dtype: float32 arrays are widened
first, where the reference would take np.mean, np.std, the severity quotient, the squares and the history's
cumsum in float32 (over 1e5 samples that cumsum is visibly lossy). Parity is defined against the reference
called on float64 arrays. (2) The reference's hash cache (:56-69) returns what a recomputation would and is
not reproduced; enable_caching and cache_max_age_frames are accepted and ignored.

Limits: at most 4096 bins between min_frequency and max_frequency (UnsupportedError above), at most 64 modes
per frame are returned (the strongest; a warning is logged when the device counted more), histories of 2 to
2^20 samples. A history whose regression range has fewer than 3 points, or that holds a non-finite sample, is
finished with numpy on the host: its result is the reference's own. sustained_peaks_history is kept as the
reference keeps it: an empty deque nothing fills.
"""
from __future__ import annotations

import ctypes as C
import logging
from collections import deque
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

logger = logging.getLogger(__name__)

MAX_MODES, ROWS, COLS, MAX_BINS, RT60_COLS, MAX_HISTORY = 64, 65, 8, 4096, 8, 1 << 20
MODE_COLUMNS = ("frequency", "magnitude", "q_factor", "severity", "type", "prominence", "bandwidth", "bin")
RT60_COLUMNS = ("curve0", "idx5", "idx10", "idx35", "slope", "intercept", "r_squared", "flags")
FLAG_NONFINITE, FLAG_FLAT, FLAG_TRUNCATED = 1, 2, 4
RT_NONFINITE, RT_NO_RANGE, RT_FEW_POINTS, RT_NO_DECAY = 1, 2, 4, 8
TYPE_NAMES = ("axial_length", "axial_width", "axial_height", "tangential", "oblique")
RT60_METHODS = ("schroeder", "edt", "simple")


def type_name(code: int) -> str:
    """The device's type code (base + 8 harmonic) as the reference's string."""
    base, harmonic = int(code) & 7, int(code) >> 3
    return f"{TYPE_NAMES[base]}_H{harmonic}" if harmonic else TYPE_NAMES[base]


@dataclass
class RoomModeConfig:
    min_frequency: float = 30.0
    max_frequency: float = 300.0
    peak_threshold_multiplier: float = 2.0
    minimum_prominence_std: float = 1.0
    min_q_factor: float = 0.5
    max_q_factor: float = 100.0
    minimum_severity: float = 0.3
    temperature_celsius: float = 20.0
    humidity_percent: float = 50.0
    enable_caching: bool = True
    cache_max_age_frames: int = 10
    rt60_method: str = "schroeder"
    min_audio_history: int = 30
    room_length_hint: float = 0.0
    room_width_hint: float = 0.0
    room_height_hint: float = 0.0

    def __post_init__(self):
        checks = (
            (self.min_frequency >= self.max_frequency, "min_frequency must be less than max_frequency"),
            (self.peak_threshold_multiplier <= 0, "peak_threshold_multiplier must be positive"),
            (self.minimum_prominence_std < 0, "minimum_prominence_std must be non-negative"),
            (self.min_q_factor >= self.max_q_factor, "min_q_factor must be less than max_q_factor"),
            (not 0 <= self.minimum_severity <= 1, "minimum_severity must be between 0 and 1"),
            (not -50 <= self.temperature_celsius <= 50, "temperature_celsius must be between -50 and 50"),
            (not 0 <= self.humidity_percent <= 100, "humidity_percent must be between 0 and 100"),
            (self.cache_max_age_frames < 0, "cache_max_age_frames must be non-negative"),
            (self.rt60_method not in RT60_METHODS, "rt60_method must be one of: schroeder, edt, simple"),
            (self.min_audio_history < 1, "min_audio_history must be at least 1"),
        )
        for failed, message in checks:
            if failed:
                raise ValueError(message)


class RoomModeAnalyzer:
    def __init__(self, sample_rate: int = 48000, config: Optional[RoomModeConfig] = None, device: int = 0):
        self._host_init(sample_rate, config)
        self._eng = utility_engine(sample_rate, device)

    def _host_init(self, sample_rate: int = 48000, config: Optional[RoomModeConfig] = None) -> None:
        """The state that needs no device (the tests drive the host methods on it alone)."""
        self.sample_rate = sample_rate
        self.config = config or RoomModeConfig()
        self.sustained_peaks_history = deque(maxlen=300)
        self._audio_history = deque(maxlen=self.config.min_audio_history * 2)
        self._configured = None

    # -- host scalar logic --
    def get_speed_of_sound(self, temperature_c: Optional[float] = None,
                           humidity_percent: Optional[float] = None) -> float:
        """:241-255."""
        temp = self.config.temperature_celsius if temperature_c is None else temperature_c
        humidity = self.config.humidity_percent if humidity_percent is None else humidity_percent
        return 331.3 * np.sqrt(1 + temp / 273.15) + 0.02 * humidity

    def _get_room_dimensions(self) -> Optional[Dict[str, float]]:
        c = self.config
        if c.room_length_hint > 0 and c.room_width_hint > 0 and c.room_height_hint > 0:
            return {"length": c.room_length_hint, "width": c.room_width_hint, "height": c.room_height_hint}
        return None

    def _expected_frequencies(self, dims: Optional[Dict[str, float]]) -> Optional[List[float]]:
        """The six frequencies of :199-223: the axial fundamentals, then the tangential ones; None without a
        complete set of positive dimensions."""
        if not dims or not all(d > 0 for d in dims.values()):
            return None
        c = self.get_speed_of_sound()
        ln, wd, ht = dims.get("length", 10), dims.get("width", 8), dims.get("height", 3)
        out = [c / (2 * ln), c / (2 * wd), c / (2 * ht)]
        for a, b in ((dims["length"], dims["width"]), (dims["length"], dims["height"]),
                     (dims["width"], dims["height"])):
            out.append(c * np.sqrt((1 / (2 * a)) ** 2 + (1 / (2 * b)) ** 2))
        return [float(v) for v in out]

    def classify_room_mode(self, frequency: float, room_dimensions: Optional[Dict] = None) -> str:
        """:191-239."""
        exp = self._expected_frequencies(room_dimensions)
        if exp:
            for harmonic in (1, 2, 3):
                for name, fundamental in zip(TYPE_NAMES[:3], exp[:3]):
                    if abs(frequency - fundamental * harmonic) < 5:
                        return f"{name}_H{harmonic}"
            if any(abs(frequency - f) < 10 for f in exp[3:]):
                return "tangential"
        for name, (lo, hi) in zip(TYPE_NAMES, ((30, 80), (80, 120), (120, 200), (200, 300))):
            if lo <= frequency <= hi:
                return name
        return "oblique"

    def estimate_q_factor(self, magnitudes: np.ndarray, freqs: np.ndarray, peak_idx: int) -> float:
        """:143-189 on the host (the device does the same per peak)."""
        n = len(magnitudes)
        if peak_idx <= 0 or peak_idx >= n - 1:
            return 1.0
        half = magnitudes[peak_idx] / np.sqrt(2)
        centre = freqs[peak_idx]
        edges = [centre, centre]
        for side, walk in enumerate((range(peak_idx - 1, -1, -1), range(peak_idx + 1, n))):
            for i in walk:
                if magnitudes[i] <= half:
                    a = i if side == 0 else i - 1  # the pair (a, a + 1) straddles the crossing
                    y1, y2, f1, f2 = magnitudes[a], magnitudes[a + 1], freqs[a], freqs[a + 1]
                    edges[side] = f1 + (half - y1) * (f2 - f1) / (y2 - y1)
                    break
        bandwidth = edges[1] - edges[0]
        q = centre / bandwidth if bandwidth > 0 else 50.0
        return min(self.config.max_q_factor, max(self.config.min_q_factor, q))

    def estimate_room_dimensions(self, room_modes: List[Dict[str, Any]]) -> Dict[str, float]:
        """:269-327."""
        c = self.get_speed_of_sound()
        dims = {"length": 0.0, "width": 0.0, "height": 0.0, "confidence": 0.0}
        found = 0
        for key in ("length", "width", "height"):
            group = [m for m in room_modes if f"axial_{key}" in m["type"]]
            found += len(group)
            if not group:
                continue
            lowest = min(group, key=lambda m: m["frequency"])
            harmonic = 1
            if "_H" in lowest["type"]:
                try:
                    harmonic = int(lowest["type"].split("_H")[1])
                except ValueError:
                    harmonic = 1
            dims[key] = c / (2 * lowest["frequency"] / harmonic)
        if found > 0:
            avg_q = np.mean([m["q_factor"] for m in room_modes]) if room_modes else 1.0
            dims["confidence"] = (min(1.0, found / 6.0) + min(1.0, avg_q / 20.0)) / 2
        return dims

    def update_audio_history(self, audio_chunk) -> None:
        """:329-332."""
        if audio_chunk is not None and len(audio_chunk) > 0:
            self._audio_history.append(np.array(audio_chunk, copy=True))

    # -- the device part --
    def _configure(self, freqs: np.ndarray) -> None:
        hints = self._expected_frequencies(self._get_room_dimensions())
        c = self.config
        key = (freqs.tobytes(), tuple(hints or ()), float(self.sample_rate), c.min_frequency, c.max_frequency,
               c.peak_threshold_multiplier, c.minimum_prominence_std, c.min_q_factor, c.max_q_factor,
               c.minimum_severity)
        if self._configured == key:
            return
        cfg = L.RoomConfig(float(self.sample_rate), c.min_frequency, c.max_frequency, c.peak_threshold_multiplier,
                           c.minimum_prominence_std, c.min_q_factor, c.max_q_factor, c.minimum_severity)
        h = np.asarray(hints or [0.0] * 6, np.float64)
        self._eng._check(L.lib().omega_room_configure(self._eng._ctx, C.byref(cfg), freqs.ctypes.data, len(freqs),
                                                      h.ctypes.data))
        self._configured = key

    def analyze_spectra(self, spectra, freqs):
        """spectra [F, n_bins] float32 / float64 (host numpy, or a device torch tensor whose rows may overlap),
        freqs [n_bins] strictly increasing. Returns the raw rows [F, 65, 8] float64 (row 0 the header count,
        flags, mean, std; then MODE_COLUMNS), numpy for host input and a device tensor for device input."""
        freqs = np.ascontiguousarray(np.asarray(freqs.cpu() if _is_torch(freqs) else freqs), np.float64)
        message = "spectra must be [F, len(freqs)]"
        dev = _is_torch(spectra)
        if dev and (spectra.dim() != 2 or spectra.shape[1] != len(freqs)):  # (refused before any copy)
            raise ValueError(message)
        spectra, spec_ptr, stride, f64 = M.rows(spectra, dev, message, audio=True)
        F, nb = spectra.shape
        if nb != len(freqs):
            raise ValueError(message)
        self._configure(freqs)
        out = M.alloc(spectra, (F, ROWS, COLS), np.float64)
        if F:
            M.call(self._eng, L.lib().omega_room_modes, spectra, spec_ptr, f64, stride, F, _ptr(out))
        return out

    @staticmethod
    def modes_from_rows(rows) -> List[Dict[str, Any]]:
        """One frame's raw rows [65, 8] as the reference's list of dicts."""
        count = int(rows[0, 0])
        if count > MAX_MODES:
            logger.warning("room modes: %d modes found, the strongest %d returned", count, MAX_MODES)
        return [{"frequency": float(r[0]), "magnitude": float(r[1]), "q_factor": float(r[2]), "severity": float(r[3]),
                 "type": type_name(r[4]), "prominence": float(r[5]), "bandwidth": float(r[6])}
                for r in rows[1:1 + min(count, MAX_MODES)]]

    def detect_room_modes_batch(self, spectra, freqs) -> List[List[Dict[str, Any]]]:
        rows = self.analyze_spectra(spectra, freqs)
        rows = rows.cpu().numpy() if _is_torch(rows) else rows
        return [self.modes_from_rows(r) for r in rows]

    def detect_room_modes(self, fft_data, freqs) -> List[Dict[str, Any]]:
        """:38-141 for one spectrum."""
        if fft_data is None or freqs is None:
            return []
        if len(fft_data) != len(freqs):
            logger.error("FFT data and frequency arrays must have same length")
            return []
        if len(fft_data) == 0:
            return []
        one = fft_data[None, :] if _is_torch(fft_data) else np.asarray(fft_data)[None, :]
        rows = self.analyze_spectra(one, freqs)
        rows = rows.cpu().numpy() if _is_torch(rows) else rows
        if int(rows[0, 0, 1]) & FLAG_NONFINITE:
            logger.warning("Invalid values in input arrays")
        return self.modes_from_rows(rows[0])

    def analyze_histories(self, audio, frame_len: int = 0):
        """audio [S, L] float32 / float64 (host numpy, or a device torch tensor whose rows may overlap). Returns
        (rows [S, 8] in RT60_COLUMNS order, energies [S, L / frame_len] or None), float64."""
        W = int(frame_len)
        if self._configured is None:  # (the decay fit reads the sample rate alone)
            self._configure(np.linspace(0.0, self.sample_rate / 2, 512))
        audio, audio_ptr, stride, f64 = M.rows(audio, _is_torch(audio), "audio must be [S, L]", audio=True)
        S, n = audio.shape
        rows = M.alloc(audio, (S, RT60_COLS), np.float64)
        en = M.alloc(audio, (S, n // W), np.float64) if W else None
        if S:
            M.call(self._eng, L.lib().omega_room_decay, audio, audio_ptr, f64, stride, n, W, S, _ptr(rows), _ptr(en))
        return rows, en

    # -- RT60: the device rows finished on the host --
    def calculate_rt60_estimate(self, method: Optional[str] = None) -> Dict[str, float]:
        """:334-354."""
        calc = self.config.rt60_method if method is None else method
        if len(self._audio_history) < self.config.min_audio_history:
            return {"rt60": 0.0, "confidence": 0.0, "method": calc}
        try:
            history = [np.asarray(a, np.float64) for a in self._audio_history]  # (float32 is widened first)
            audio = np.concatenate(history)
            W = len(history[0]) if all(len(a) == len(history[0]) for a in history) else 0
            row, en = self.analyze_histories(audio[None, :], W)
            row, en = row[0], (en[0] if W else np.array([np.sum(a ** 2) for a in history]))
            if calc == "schroeder":
                return self.finish_schroeder(row, audio)
            if calc == "edt":
                return self.finish_edt(row, len(audio), audio)
            if int(row[7]) & RT_NONFINITE:
                en = np.array([np.sum(a ** 2) for a in history])
            return self.finish_simple(en, len(history[0]))
        except Exception as e:  # (the reference's own convention, :352-354)
            logger.error("RT60 calculation error: %s", e)
            return {"rt60": 0.0, "confidence": 0.0, "error": str(e), "method": calc}

    def _host_curve_db(self, audio: np.ndarray) -> np.ndarray:
        curve = np.maximum(np.cumsum((audio ** 2)[::-1])[::-1], 1e-10)
        return 10 * np.log10(curve / curve[0])

    def finish_schroeder(self, row, audio: Optional[np.ndarray] = None) -> Dict[str, float]:
        """:373-420 from one device row; `audio` serves the rows the host finishes."""
        flags = int(row[7])
        if flags & (RT_NONFINITE | RT_FEW_POINTS):
            db = self._host_curve_db(audio)
            below5, below35 = np.flatnonzero(db <= -5), np.flatnonzero(db <= -35)
            if len(below5) == 0 or len(below35) == 0 or below35[0] <= below5[0]:
                return {"rt60": 0.5, "confidence": 0.1, "method": "schroeder"}
            try:
                t = np.arange(len(db)) / self.sample_rate
                sl = slice(below5[0], below35[0])
                coeffs = np.polyfit(t[sl], db[sl], 1)
                slope = coeffs[0]
                resid = db[sl] - np.polyval(coeffs, t[sl])
                r_squared = 1 - np.sum(resid ** 2) / np.sum((db[sl] - np.mean(db[sl])) ** 2)
            except (IndexError, ValueError):
                return {"rt60": 0.5, "confidence": 0.0, "method": "schroeder"}
        elif flags & RT_NO_RANGE:
            return {"rt60": 0.5, "confidence": 0.1, "method": "schroeder"}
        else:
            slope, r_squared = np.float64(row[4]), np.float64(row[6])
        rt60 = -60.0 / slope if slope < 0 else 0.5
        return {"rt60": min(5.0, max(0.05, rt60)), "confidence": max(0.0, min(1.0, r_squared)),
                "method": "schroeder", "slope": slope, "r_squared": r_squared}

    def finish_edt(self, row, n: int, audio: Optional[np.ndarray] = None) -> Dict[str, float]:
        """:433-458 from one device row of a history of n samples."""
        if int(row[7]) & RT_NONFINITE:
            below = np.flatnonzero(self._host_curve_db(audio) <= -10)
            idx10 = int(below[0]) if len(below) else n
        else:
            idx10 = int(row[2])
        if idx10 >= n:
            return {"rt60": 0.5, "confidence": 0.1, "method": "edt"}
        with np.errstate(divide="ignore"):
            slope = -10.0 / (np.float64(idx10) / self.sample_rate)
            edt = -60.0 / slope if slope < 0 else 0.5
        return {"rt60": min(5.0, max(0.05, edt)), "confidence": 0.7, "method": "edt"}

    def finish_simple(self, energies, frame_len: int) -> Dict[str, float]:
        """:465-500 from the frames' sums of squares."""
        energies = [float(e) for e in energies]
        top = max(energies)
        if top == 0:
            return {"rt60": 0.0, "confidence": 0.0, "method": "simple"}
        db = 10 * np.log10(np.array(energies) / top + 1e-10)
        frame_duration = frame_len / self.sample_rate
        reached = np.flatnonzero(db <= -60)
        if len(reached):
            return {"rt60": min(3.0, max(0.1, reached[0] * frame_duration)), "confidence": 0.5, "method": "simple"}
        if len(db) > 2:
            slope = np.polyfit(np.arange(len(db)), db, 1)[0]
            if slope < 0:
                return {"rt60": min(3.0, max(0.1, -60 / slope * frame_duration)), "confidence": 0.3,
                        "method": "simple"}
        return {"rt60": 0.5, "confidence": 0.1, "method": "simple"}
