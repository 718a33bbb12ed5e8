"""HarmonicAnalyzer on the MI355X: detect_harmonic_series
(omega4/panels/harmonic_analysis.py:193-333) with the HarmonicMetrics it calls
(omega4/analyzers/harmonic_metrics.py:51-357) -- peak picking, harmonic series, THD, THD+N, spectral
shape, HNR and the LPC formants per frame -- over libomega.so's omega_harmonic_analyze.

``analyze_frames(spectra, freqs, frames)`` analyses a batch of one stream's frames in one launch (host
numpy or device torch); ``detect_harmonic_series(fft_data, freqs, audio_data)`` returns the reference's
dict for one frame, the per-series ``harmonics`` lists rebuilt on the host from the device's bins. The
previous spectrum the flux compares with lives in the context (``reset()`` forgets it); the two
60-deep histories are kept here. Device batches follow the facades' common row rule (_marshal.rows): rows
that overlap or belong to a wider table are read in place; a batch with ``stride(0) < 1`` and F > 1 (an
``expand`` of one row) is copied and analysed, where this facade once left it to the library to refuse.

Instrument identification (:335-431) is scalar host work on at most three series. The profile table is
data the caller supplies (``HarmonicAnalyzer(fs, instrument_profiles=reference.instrument_profiles)``);
without one ``instrument_matches`` is ``[]``. The scoring is restated as the reference behaves: a score
is only ever assigned inside its ``"inharmonicity" in profile and len(harmonics) > 3`` branch, so a
series with three or fewer harmonics scores 0 for every instrument and the 20 % bonus multiplies 0.

There is no CPU fallback: a shape the library does not build (bins outside 16..8193, audio outside
15..8192 samples) raises UnsupportedError with the library's message.
"""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

COLUMNS = ("series_count", "dominant_fundamental", "thd", "thd_plus_noise", "spectral_centroid", "spectral_spread",
           "spectral_flux", "spectral_rolloff", "inharmonicity", "hnr_db", "formant_count", "F1", "F2", "F3", "F4",
           "flags")
FLAG_NOT_CONVERGED, FLAG_NONFINITE = 1, 2
MAX_HARMONIC = 16
SERIES_COLS = 1 + MAX_HARMONIC

# average vowel formants (Hz) and per-voice formant ranges, as HarmonicMetrics tabulates them
VOWEL_FORMANTS = {"a": (730, 1090, 2440), "e": (530, 1840, 2480), "i": (270, 2290, 3010), "o": (570, 840, 2410),
                  "u": (300, 870, 2240)}
FORMANT_RANGES = {"male": ((200, 900), (700, 2300), (1500, 3500), (2500, 4500)),
                  "female": ((250, 1000), (800, 2800), (1800, 4000), (3000, 5000)),
                  "child": ((300, 1100), (900, 3200), (2000, 4500), (3500, 5500))}


def _tables(values):
    return {k: {f"F{i + 1}": x for i, x in enumerate(v)} for k, v in values.items()}


class HarmonicAnalyzer:
    def __init__(self, sample_rate: int = 48000, instrument_profiles: Optional[Dict[str, Dict[str, Any]]] = None,
                 device: int = 0, max_series: int = 16):
        if not sample_rate > 0:
            raise ValueError("Sample rate must be positive")
        self.sample_rate = sample_rate
        self.nyquist = sample_rate / 2
        self.instrument_profiles = dict(instrument_profiles) if instrument_profiles else {}
        self.max_series = int(max_series)
        self.harmonic_history = deque(maxlen=30)
        self.instrument_confidence: Dict[str, float] = {}
        self.spectral_centroid_history = deque(maxlen=60)
        self.thd_history = deque(maxlen=60)
        self.metrics = HarmonicMetrics(sample_rate, device=device)
        self._eng = utility_engine(sample_rate, device)
        self._freqs: Optional[np.ndarray] = None

    # -- the device part --
    def _configure(self, freqs, n_bins: int) -> np.ndarray:
        fr = np.ascontiguousarray(freqs.detach().cpu().numpy() if _is_torch(freqs) else freqs, np.float64)
        if fr.ndim != 1 or fr.shape[0] != n_bins:
            raise ValueError(f"freqs must hold one entry per spectrum bin ({n_bins}), got shape {fr.shape}")
        if self._freqs is None or self._freqs.shape != fr.shape or not np.array_equal(self._freqs, fr):
            cfg = L.HarmonicConfig(int(self.sample_rate), int(n_bins), self.max_series)
            self._freqs = None
            self._eng._check(L.lib().omega_harmonic_configure(self._eng._ctx, C.byref(cfg), fr.ctypes.data))
            self._freqs = fr.copy()
        return self._freqs

    def reset(self) -> None:
        """Forget the previous spectrum (the next frame's flux is 0)."""
        self._eng._check(L.lib().omega_harmonic_reset(self._eng._ctx))

    def analyze_frames(self, spectra, freqs, frames=None):
        """spectra [F, K] float32, freqs [K], frames [F, m] float32 / float64 or None (no formants) -- host
        numpy, or device torch tensors whose rows may overlap (an ``unfold`` view of a stream). Returns
        (out [F, 16] float64 in COLUMNS order, series_bins [F, max_series, 17] int32, series_strength
        [F, max_series] float64): numpy for host input, device tensors for device input. The frames are one
        stream in order: the flux of frame f compares with frame f-1, that of frame 0 with the last frame of
        the previous call."""
        dev = _is_torch(spectra)
        if dev and frames is not None and not _is_torch(frames):
            raise ValueError(M.MIXED_SIDES)
        spectra, spec_ptr, spec_stride, _ = M.rows(spectra, dev, "spectra must be [F, K]")
        F, K = spectra.shape
        self._configure(freqs, K)
        audio_ptr, f64, m, audio_stride = None, 0, 0, 1  # (no audio: a null pointer, and any positive stride)
        if frames is not None:
            frames, audio_ptr, audio_stride, f64 = M.rows(frames, dev, "frames must be [F, m]", audio=True)
            if frames.shape[0] != F:
                raise ValueError("frames must be [F, m]")
            m = frames.shape[1]
        out = M.alloc(spectra, (F, len(COLUMNS)), np.float64)
        sb = M.alloc(spectra, (F, self.max_series, SERIES_COLS), np.int32)
        ss = M.alloc(spectra, (F, self.max_series), np.float64)
        M.call(self._eng, L.lib().omega_harmonic_analyze, spectra, spec_ptr, spec_stride, audio_ptr, f64, m,
               audio_stride, F, _ptr(out), _ptr(sb), _ptr(ss))
        return out, sb, ss

    # -- the reference's surface --
    @staticmethod
    def series_dicts(spec: np.ndarray, freqs: np.ndarray, bins: np.ndarray, strength: np.ndarray, count: int
                     ) -> List[Dict[str, Any]]:
        """The reference's ``harmonic_series`` entries (:308-333) for one frame from the device's rows: the
        values are table look-ups and the float32 quotient the reference forms."""
        spec = np.asarray(spec, np.float32)
        out = []
        for row, s in zip(bins[:count], strength[:count]):
            f0, fmag = freqs[row[0]], spec[row[0]]
            hs = [{"number": n, "expected_freq": f0 * n, "actual_freq": freqs[b], "magnitude": spec[b],
                   "relative_strength": spec[b] / (fmag + 1e-10)}
                  for n, b in enumerate(row[1:], start=1) if b >= 0]
            out.append({"fundamental": f0, "harmonics": hs, "strength": float(s), "harmonic_count": len(hs)})
        return out

    def detect_harmonic_series(self, fft_data, freqs, audio_data=None) -> Dict[str, Any]:
        """:193-279 for one frame."""
        spec = np.ascontiguousarray(fft_data, np.float32)
        audio = None
        if audio_data is not None and len(audio_data) > 14:
            audio = np.asarray(audio_data)[None, :]
        out, sb, ss = self.analyze_frames(spec[None, :], freqs, audio)
        row = out[0]
        found = self.series_dicts(spec, self._freqs, sb[0], ss[0], min(int(row[0]), self.max_series))
        result = {"harmonic_series": found, "instrument_matches": self.identify_instruments(found[:3]),
                  "dominant_fundamental": found[0]["fundamental"] if found else 0}
        for k, name in enumerate(COLUMNS[2:10], start=2):
            result[name] = float(row[k])
        result["formants"] = [float(v) for v in row[11:11 + int(row[10])]]
        result["hnr_db"] = result.pop("hnr_db")  # (the reference's key order: formants before hnr_db)
        self.spectral_centroid_history.append(result["spectral_centroid"])
        self.thd_history.append(result["thd"])
        return result

    def identify_instruments(self, harmonic_series_list: List[Dict]) -> List[Dict[str, Any]]:
        """:335-361: the mean score per instrument over the given series, above 0.3, best first."""
        scores: Dict[str, list] = {}
        for series in harmonic_series_list:
            for name, profile in self.instrument_profiles.items():
                scores.setdefault(name, []).append(
                    self.calculate_instrument_match_score(series["fundamental"], series["harmonics"], profile))
        matches = []
        for name, vals in scores.items():
            mean = np.mean(vals) if vals else 0.0
            if mean > 0.3:
                matches.append({"instrument": name, "confidence": mean, "match_count": len(vals)})
        matches.sort(key=lambda e: e["confidence"], reverse=True)
        return matches

    def calculate_instrument_match_score(self, fundamental: float, harmonics: List[Dict], profile: Dict) -> float:
        """:363-414 as it behaves (see the module docstring)."""
        lo, hi = profile["fundamental_range"]
        if not lo <= fundamental <= hi:
            return 0.0
        if "inharmonicity" not in profile or len(harmonics) <= 3:
            return 0.0
        by_number = {h["number"]: h for h in harmonics}
        total, n = 0.0, 0
        for i, expected in enumerate(profile["harmonic_pattern"]):
            h = by_number.get(i + 1)
            if h is not None:
                total += 1.0 - min(abs(expected - h["relative_strength"]), 1.0)
                n += 1
        return total / n if n else 0.0


class HarmonicMetrics:
    """The reference's HarmonicMetrics surface (harmonic_metrics.py:51-357), stateless like it: every
    method evaluates its one frame through omega_harmonic_metrics on a context of its own, so a call never
    touches an analyzer's previous-spectrum state. The device call evaluates thd, thd_plus_noise,
    inharmonicity and hnr_db for the fundamental the caller names, and centroid / spread / rolloff / the
    formants for any spectrum, with or without a harmonic series. What the kernels fix is reported, not
    emulated on the CPU: num_harmonics other than the defaults (5, 10 for the inharmonicity), a rolloff
    percentage other than 0.85, an LPC order other than 14, a `centroid` argument that is not the
    spectrum's own and flux operands of different lengths raise UnsupportedError. The vowel lookup is host
    logic."""

    def __init__(self, sample_rate: int = 48000, device: int = 0):
        if not sample_rate > 0:
            raise ValueError("Sample rate must be positive")
        self.sample_rate = sample_rate
        self.nyquist = sample_rate / 2
        self.formant_ranges = _tables(FORMANT_RANGES)
        self.vowel_formants = _tables(VOWEL_FORMANTS)
        self._own: Optional[HarmonicAnalyzer] = None  # (a context of its own, opened at the first device call)
        self._device = device

    def _row(self, fft_data, freqs, fundamental=0.0, previous=None, audio=None) -> np.ndarray:
        if self._own is None:
            self._own = HarmonicAnalyzer(self.sample_rate, device=self._device, max_series=1)
        an = self._own
        spec = np.ascontiguousarray(fft_data, np.float32)
        if spec.ndim != 1:
            raise ValueError("fft_data must be one spectrum")
        an._configure(freqs, spec.shape[0])
        prev = None if previous is None else np.ascontiguousarray(previous, np.float32)
        ap, f64, m = None, 0, 0
        if audio is not None:
            audio = np.asarray(audio)
            audio = np.ascontiguousarray(audio if audio.dtype in (np.float32, np.float64) else audio.astype(np.float64))
            ap, f64, m = audio.ctypes.data, int(audio.dtype == np.float64), audio.shape[0]
        out = np.empty(len(COLUMNS), np.float64)
        an._eng._check(L.lib().omega_harmonic_metrics(an._eng._ctx, spec.ctypes.data, None if prev is None else prev.ctypes.data,
                                                      ap, f64, m, float(fundamental), out.ctypes.data, L.MEM_HOST))
        return out

    @staticmethod
    def _only(what, got, built):
        if got != built:
            raise L.UnsupportedError(L.EUNSUP, f"harmonic metrics: {what} {got!r} (the kernels build {built!r})")

    def calculate_thd(self, fft_data, freqs, fundamental_freq, num_harmonics: int = 5) -> float:
        self._only("num_harmonics", num_harmonics, 5)
        return float(self._row(fft_data, freqs, fundamental_freq)[2])

    def calculate_thd_plus_noise(self, fft_data, freqs, fundamental_freq, num_harmonics: int = 5) -> float:
        return float(self._row(fft_data, freqs, fundamental_freq)[3])  # (the reference never reads num_harmonics here)

    def detect_formants_lpc(self, audio_data, order: int = 14) -> List[float]:
        self._only("LPC order", order, 14)
        if len(audio_data) < order + 1:
            return []
        row = self._row(np.zeros(16, np.float32), np.linspace(0.0, self.nyquist, 16), audio=audio_data)
        return [float(v) for v in row[11:11 + int(row[10])]]

    def calculate_spectral_centroid(self, fft_data, freqs) -> float:
        return float(self._row(fft_data, freqs)[4])

    def calculate_spectral_spread(self, fft_data, freqs, centroid: Optional[float] = None) -> float:
        row = self._row(fft_data, freqs)
        if centroid is not None:
            self._only("centroid", float(centroid), float(row[4]))
        return float(row[5])

    def calculate_spectral_flux(self, current_fft, previous_fft) -> float:
        self._only("previous spectrum length", len(previous_fft), len(current_fft))
        n = len(current_fft)
        fr = self._own._freqs if self._own is not None and self._own._freqs is not None and len(self._own._freqs) == n \
            else np.arange(n, dtype=np.float64)
        return float(self._row(current_fft, fr, previous=previous_fft)[6])

    def calculate_spectral_rolloff(self, fft_data, freqs, percentage: float = 0.85) -> float:
        self._only("rolloff percentage", percentage, 0.85)
        return float(self._row(fft_data, freqs)[7])

    def calculate_harmonic_to_noise_ratio(self, fft_data, freqs, fundamental_freq, num_harmonics: int = 5) -> float:
        self._only("num_harmonics", num_harmonics, 5)
        return float(self._row(fft_data, freqs, fundamental_freq)[9])

    def calculate_inharmonicity(self, fft_data, freqs, fundamental_freq, num_harmonics: int = 10) -> float:
        self._only("num_harmonics", num_harmonics, 10)
        return float(self._row(fft_data, freqs, fundamental_freq)[8])

    def detect_vowel_from_formants(self, formants: List[float]) -> Tuple[str, float]:
        """The vowel whose tabulated (F1, F2) lies nearest, and 1 - distance / 1000 clamped at 0."""
        if len(formants) < 2:
            return "unknown", 0.0
        best, dist = "unknown", float("inf")
        for vowel, f in self.vowel_formants.items():
            d = np.sqrt((formants[0] - f["F1"]) ** 2 + (formants[1] - f["F2"]) ** 2)
            if d < dist:
                best, dist = vowel, d
        return best, max(0, 1 - dist / 1000)
