"""HipHopDetector on the MI355X: the per-frame array work of
HipHopDetector.analyze (omega4/panels/hip_hop_detector.py:94-384) over libomega.so's omega_hiphop_features,
and its scalar logic (:386-486) on the host.

``analyze_frames(spectra, freqs, frames)`` evaluates a batch of independent frames in one launch (host numpy
or device torch) and returns the rows in COLUMNS order plus the kept kick-envelope peaks;
``analyze(audio_chunk, fft_data, freqs, drum_info)`` returns the reference's dict for one frame: same keys,
same insertion order, ``spectral_tilt`` and ``vocal_presence`` as numpy float32 where the reference's are.
``result_from_row(row, drum_info)`` is the host part alone. The three band-pass cascades (sub-bass 20-60 Hz,
kick 40-100 Hz, hi-hat 3000-min(10000, 0.9 fs/2) Hz; scipy.signal.butter(4, ..., 'bandpass', output='sos'))
are designed by the library; every frame is filtered from the zero state, as the reference does, so the
device keeps no state and the 30-deep histories live here.

The scalar parts are restated as the reference behaves: ``kick_detected`` and the kick magnitude come from
``drum_info``; ``feature_weights`` names ``sub_bass`` and ``kick_pattern`` while the features are called
``sub_bass_presence`` and ``kick_pattern_score``, so those two weights never count (a caller may assign
another table to the attribute). A silent frame (rms < 0.001) returns the fixed dict and leaves the
histories untouched; so does a frame the device flags as non-finite.

The result feeds the genre row::

    hh = HipHopDetector(48000)
    clf = GenreClassifier(48000, genre_patterns=...)
    features = clf.extract_features(fft_data, audio_chunk, freqs, drum_info, harmonic_info)
    probs = clf.classify(features, hip_hop_confidence=hh.analyze(audio_chunk, fft_data, freqs, drum_info)['confidence'])

There is no CPU fallback: a shape the library does not build (bins outside 16..8193, a frame length that is
not a power of two 64..8192, a rate below 8000 Hz) raises UnsupportedError with the library's message.
"""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Any, Dict, Optional

import numpy as np

from . import _lib as L
from ._marshal import _is_torch
from .engine import utility_engine

COLUMNS = ("rms", "sub_bass_presence", "kick_peak_count", "kick_pattern_factor", "hihat_zero_crossings",
           "hihat_density", "spectral_tilt", "vocal_peak_count", "vocal_presence", "flags", "sub_bass_rms",
           "hihat_rms", "envelope_threshold", "sub_bass_power", "bass_power", "total_power", "low_energy",
           "mid_energy", "high_energy", "vocal_energy", "core_vocal_energy", "total_energy", "tilt_branch",
           "vocal_branch")
FLAG_SILENT, FLAG_NONFINITE = 1, 2
N_PEAKS = 16
FILTERS = ("sub_bass", "kick", "hihat")
_COL = {k: i for i, k in enumerate(COLUMNS)}


class HipHopDetector:
    def __init__(self, sample_rate: int = 48000, device: int = 0):
        if not sample_rate > 0:
            raise ValueError("Sample rate must be positive")
        self._host_init(sample_rate)
        self._eng = utility_engine(sample_rate, device)

    def _host_init(self, sample_rate) -> None:
        """The state that needs no device (the tests build the host logic on it alone)."""
        self.sample_rate = sample_rate
        self.sub_bass_history = deque(maxlen=30)
        self.kick_pattern_history = deque(maxlen=30)
        self.hihat_density_history = deque(maxlen=30)
        self.spectral_tilt_history = deque(maxlen=30)
        self.confidence_history = deque(maxlen=30)
        self.subgenre_profiles = {
            "trap": {"tempo_range": (130, 170), "hihat_density": (0.7, 1.0), "sub_bass_presence": (0.8, 1.0),
                     "kick_spacing": "syncopated", "snare_pattern": "sparse", "vocal_style": "melodic_autotuned"},
            "boom_bap": {"tempo_range": (80, 100), "hihat_density": (0.3, 0.6), "sub_bass_presence": (0.4, 0.7),
                         "kick_spacing": "regular", "snare_pattern": "backbeat", "vocal_style": "rhythmic_traditional"},
            "modern": {"tempo_range": (70, 90), "hihat_density": (0.5, 0.8), "sub_bass_presence": (0.6, 0.9),
                       "kick_spacing": "varied", "snare_pattern": "trap_influenced", "vocal_style": "mixed"},
        }
        self.feature_weights = {"sub_bass": 0.25, "kick_pattern": 0.20, "hihat_density": 0.15, "spectral_tilt": 0.15,
                                "vocal_presence": 0.15, "tempo_match": 0.10}
        self._freqs: Optional[np.ndarray] = None

    # -- the device part --
    def _configure(self, freqs, n_bins: int) -> np.ndarray:
        fr = np.ascontiguousarray(freqs.detach().cpu().numpy() if _is_torch(freqs) else freqs, np.float64)
        if fr.ndim != 1 or fr.shape[0] != n_bins:
            raise ValueError(f"freqs must hold one entry per spectrum bin ({n_bins}), got shape {fr.shape}")
        if self._freqs is None or self._freqs.shape != fr.shape or not np.array_equal(self._freqs, fr):
            cfg = L.HipHopConfig(int(self.sample_rate), int(n_bins))
            # (a refused table leaves the configured one as it was)
            self._eng._check(L.lib().omega_hiphop_configure(self._eng._ctx, C.byref(cfg), fr.ctypes.data))
            self._freqs = fr.copy()
        return self._freqs

    def filter_sections(self, which: str) -> np.ndarray:
        """The configured cascade `which` ('sub_bass', 'kick', 'hihat') as scipy lays out sos: [4, 6]."""
        if self._freqs is None:
            raise ValueError("no table is configured yet: call analyze or analyze_frames first")
        out = np.empty((4, 6), np.float64)
        self._eng._check(L.lib().omega_hiphop_get_sos(self._eng._ctx, FILTERS.index(which), out.ctypes.data))
        return out

    def analyze_frames(self, spectra, freqs, frames):
        """spectra [F, K] float32, freqs [K], frames [F, m] float32 / float64 -- host numpy, or device torch
        tensors whose rows may overlap (an ``unfold`` view of a stream; a strided view of wider spectra).
        Returns (out [F, len(COLUMNS)] float64, kick_peaks [F, 16] int32): numpy for host input, device
        tensors for device input. The frames are independent."""
        lib = L.lib()
        if _is_torch(spectra):
            import torch
            if not _is_torch(frames):
                raise ValueError("spectra and frames must both be device tensors or both host arrays")
            if spectra.dtype != torch.float32:
                spectra = spectra.float()
            if spectra.dim() != 2 or frames.dim() != 2 or frames.shape[0] != spectra.shape[0]:
                raise ValueError("spectra must be [F, K] and frames [F, m]")
            if spectra.stride(1) != 1 or (spectra.shape[0] > 1 and spectra.stride(0) < 1):
                spectra = spectra.contiguous()
            if frames.dtype not in (torch.float32, torch.float64):
                frames = frames.double()
            if frames.stride(1) != 1 or (frames.shape[0] > 1 and frames.stride(0) < 1):
                frames = frames.contiguous()
            F, K = spectra.shape
            m = frames.shape[1]
            self._check_shape(K, m)
            self._configure(freqs, K)
            out = torch.empty((F, len(COLUMNS)), dtype=torch.float64, device=spectra.device)
            kp = torch.empty((F, N_PEAKS), dtype=torch.int32, device=spectra.device)
            self._eng._bind_stream(spectra)
            self._eng._check(lib.omega_hiphop_features(
                self._eng._ctx, spectra.data_ptr(), spectra.stride(0) if F > 1 else K, frames.data_ptr(),
                int(frames.dtype == torch.float64), m, frames.stride(0) if F > 1 else m, F, out.data_ptr(),
                kp.data_ptr(), L.MEM_DEVICE))
            return out, kp
        spectra = np.ascontiguousarray(spectra, np.float32)
        frames = np.asarray(frames)
        frames = np.ascontiguousarray(frames if frames.dtype in (np.float32, np.float64) else frames.astype(np.float64))
        if spectra.ndim != 2 or frames.ndim != 2 or frames.shape[0] != spectra.shape[0]:
            raise ValueError("spectra must be [F, K] and frames [F, m]")
        F, K = spectra.shape
        m = frames.shape[1]
        self._check_shape(K, m)
        self._configure(freqs, K)
        out = np.empty((F, len(COLUMNS)), np.float64)
        kp = np.empty((F, N_PEAKS), np.int32)
        self._eng._check(lib.omega_hiphop_features(self._eng._ctx, spectra.ctypes.data, K, frames.ctypes.data,
                                                   int(frames.dtype == np.float64), m, m, F, out.ctypes.data,
                                                   kp.ctypes.data, L.MEM_HOST))
        return out, kp

    @staticmethod
    def _check_shape(K: int, m: int) -> None:
        # (both sizes are refused before either touches the configured table)
        if not 16 <= K <= 8193:
            raise L.UnsupportedError(L.EUNSUP, f"hiphop: {K} spectrum bins (16..8193 are built)")
        if not (64 <= m <= 8192 and m & (m - 1) == 0):
            raise L.UnsupportedError(L.EUNSUP, f"hiphop: {m} audio samples per frame (the powers of two 64..8192 "
                                               "are built)")

    # -- the reference's surface --
    def analyze(self, audio_chunk, fft_data, freqs, drum_info: Dict) -> Dict[str, Any]:
        """:94-154 for one frame."""
        out, _ = self.analyze_frames(np.asarray(fft_data)[None, :], freqs, np.asarray(audio_chunk)[None, :])
        return self.result_from_row(out[0], drum_info)

    def result_from_row(self, row, drum_info: Dict) -> Dict[str, Any]:
        """The reference's result from one device row and the caller's drum_info; updates the histories."""
        v = {k: float(row[i]) for k, i in _COL.items()}
        if int(v["flags"]) & (FLAG_SILENT | FLAG_NONFINITE):
            return {"confidence": 0.0, "features": {}, "subgenre": "unknown", "is_hip_hop": False,
                    "sub_bass_detected": False, "strong_beat": False}
        features: Dict[str, Any] = {}
        # (the values are the reference's; so are their types where min(., 1.0) hands back the Python float)
        features["sub_bass_presence"] = np.float64(v["sub_bass_presence"]) if v["sub_bass_presence"] < 1.0 else 1.0
        kick = drum_info.get("kick", {})
        kick_detected, kick_magnitude = kick.get("kick_detected", False), kick.get("magnitude", 0.0)
        if not kick_detected:
            features["kick_pattern_score"] = 0.0
        else:
            factor = np.float64(v["kick_pattern_factor"]) if int(v["kick_peak_count"]) > 1 else 0.5
            features["kick_pattern_score"] = min(factor * kick_magnitude, 1.0)
        clipped = v["hihat_rms"] / v["rms"] * 5 > 1.0
        features["hihat_density"] = v["hihat_density"] if clipped else np.float64(v["hihat_density"])
        features["spectral_tilt"] = np.float32(v["spectral_tilt"]) if int(v["tilt_branch"]) in (1, 2) else v["spectral_tilt"]
        features["vocal_presence"] = np.float32(v["vocal_presence"]) if int(v["vocal_branch"]) == 1 else v["vocal_presence"]
        features["tempo_match"] = self._check_tempo_match(drum_info)
        confidence = self._calculate_confidence(features)
        subgenre = "unknown"
        if confidence > 0.6:
            subgenre = self._detect_subgenre(features)
        self._update_history(features, confidence)
        smoothed = self._apply_temporal_smoothing()
        return {"confidence": smoothed, "features": features, "subgenre": subgenre, "is_hip_hop": smoothed > 0.5,
                "sub_bass_detected": features["sub_bass_presence"] > 0.6,
                "strong_beat": features["kick_pattern_score"] > 0.7}

    @staticmethod
    def _check_tempo_match(drum_info: Dict) -> float:
        return 0.8 if drum_info.get("kick", {}).get("kick_detected", False) else 0.3

    def _calculate_confidence(self, features: Dict[str, float]) -> float:
        confidence = 0.0
        for feature, weight in self.feature_weights.items():
            if feature in features:
                confidence += features[feature] * weight
        if confidence > 0.7:
            confidence = min(confidence * 1.2, 1.0)
        elif confidence < 0.3:
            confidence = confidence * 0.8
        return confidence

    @staticmethod
    def _detect_subgenre(features: Dict[str, float]) -> str:
        get = features.get
        scores = {}
        trap = 0.0
        if get("hihat_density", 0) > 0.7:
            trap += 0.4
        if get("sub_bass_presence", 0) > 0.8:
            trap += 0.3
        if get("tempo_match", 0) > 0.5:
            trap += 0.3
        scores["trap"] = trap
        boom_bap = 0.0
        if 0.3 <= get("hihat_density", 0) <= 0.6:
            boom_bap += 0.3
        if 0.4 <= get("sub_bass_presence", 0) <= 0.7:
            boom_bap += 0.3
        if get("kick_pattern_score", 0) > 0.8:
            boom_bap += 0.4
        scores["boom_bap"] = boom_bap
        modern = 0.5
        if get("sub_bass_presence", 0) > 0.6:
            modern += 0.2
        if get("vocal_presence", 0) > 0.6:
            modern += 0.3
        scores["modern"] = modern
        return max(scores.items(), key=lambda x: x[1])[0]

    def _update_history(self, features: Dict[str, float], confidence: float) -> None:
        self.sub_bass_history.append(features.get("sub_bass_presence", 0))
        self.kick_pattern_history.append(features.get("kick_pattern_score", 0))
        self.hihat_density_history.append(features.get("hihat_density", 0))
        self.spectral_tilt_history.append(features.get("spectral_tilt", 0))
        self.confidence_history.append(confidence)

    def _apply_temporal_smoothing(self) -> float:
        if len(self.confidence_history) == 0:
            return 0.0
        weights = np.linspace(0.5, 1.0, len(self.confidence_history))
        weights = weights / np.sum(weights)
        smoothed = np.sum(np.array(self.confidence_history) * weights)
        recent_high = sum(1 for c in list(self.confidence_history)[-10:] if c > 0.6)
        if recent_high >= 7:
            smoothed = min(smoothed * 1.1, 1.0)
        return smoothed

    def get_debug_info(self) -> Dict[str, Any]:
        return {
            "sub_bass_history": list(self.sub_bass_history),
            "kick_pattern_history": list(self.kick_pattern_history),
            "hihat_density_history": list(self.hihat_density_history),
            "spectral_tilt_history": list(self.spectral_tilt_history),
            "confidence_history": list(self.confidence_history),
            "avg_sub_bass": np.mean(self.sub_bass_history) if self.sub_bass_history else 0,
            "avg_hihat_density": np.mean(self.hihat_density_history) if self.hihat_density_history else 0,
            "current_confidence": self.confidence_history[-1] if self.confidence_history else 0,
        }

    def reset(self) -> None:
        """Forget the histories (a new stream)."""
        for h in (self.sub_bass_history, self.kick_pattern_history, self.hihat_density_history,
                  self.spectral_tilt_history, self.confidence_history):
            h.clear()
