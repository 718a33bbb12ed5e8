"""GenreClassifier on the MI355X: extract_features
(omega4/panels/genre_classification.py:175-254) with the compute_* / estimate_* helpers it calls
(:256-422, :600-783) over libomega.so's omega_genre_features, and classify (:424-597) on the host.

``extract_features_frames(spectra, freqs, frames)`` evaluates a batch of one stream's frames in one launch
(host numpy or device torch) and returns the rows in COLUMNS order plus the five distortion peak bins;
``extract_features(fft_data, audio_chunk, freqs, drum_info, harmonic_info, ...)`` returns the reference's
dict for one frame, same keys, same insertion order. The previous magnitude the flux compares with lives
in the context (``reset()`` forgets it). The device does not apply the panel's silence gate (rms < 0.001,
:852): the reference's GenreClassifier has none, so every frame is computed and advances the flux state;
the ``rms`` column lets a caller gate without a host pass.

The scalar parts stay on the host, restated as the reference behaves: percussion strength, the tempo stub
and beat regularity from ``drum_info``; harmonic complexity from ``harmonic_info`` when a series is present,
else the device's flatness value; the chroma Gini concentration, entropy and power-chord ratio; chord
change rate and key stability. ``classify`` restates the pattern scoring, the per-genre modifiers, the
3-deep history, the boosts and the softmax. The ``genre_patterns`` table is data the caller supplies
(``GenreClassifier(fs, genre_patterns=reference.genre_patterns)``); without one ``classify`` raises. The
reference's HipHopDetector is a facade of its own (omega_gpu.HipHopDetector): pass its confidence as
``hip_hop_confidence`` or Hip-Hop is scored from its pattern row, as the reference does when classify gets
no audio.

There is no CPU fallback: a shape the library does not build (bins outside 16..8193, audio outside
15..8192 samples) raises UnsupportedError with the library's message.
"""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _lib as L
from ._marshal import _is_torch
from .engine import utility_engine

COLUMNS = ("spectral_centroid", "spectral_rolloff", "rolloff_index", "zero_crossings", "spectral_bandwidth",
           "dynamic_range", "loud", "quiet", "rms", "spectral_complexity", "bass_emphasis", "vocal_presence",
           "high_freq_energy", "spectral_flux", "distortion_count", "mid_frequency_dominance", "flags")
FLAG_NONFINITE = 2
N_PEAKS = 5
GENRES = ("Rock", "Pop", "Jazz", "Classical", "Electronic", "Hip-Hop", "Metal", "Country", "R&B", "Folk")
_COL = {k: i for i, k in enumerate(COLUMNS)}


class GenreClassifier:
    def __init__(self, sample_rate: int = 48000, genre_patterns: Optional[Dict[str, Dict[str, Any]]] = None,
                 device: int = 0):
        if not sample_rate > 0:
            raise ValueError("Sample rate must be positive")
        self._host_init(sample_rate, genre_patterns)
        self._eng = utility_engine(sample_rate, device)

    def _host_init(self, sample_rate, genre_patterns=None) -> None:
        """The state that needs no device (the tests build the host logic on it alone)."""
        self.sample_rate = sample_rate
        self.genres = list(GENRES)
        self.genre_patterns = {g: dict(row) for g, row in genre_patterns.items()} if genre_patterns else {}
        self.feature_buffer = deque(maxlen=5)
        self.genre_history = deque(maxlen=3)
        self._freqs: Optional[np.ndarray] = None

    # -- the device part --
    def _configure(self, freqs, n_bins: int) -> np.ndarray:
        fr = np.ascontiguousarray(freqs.detach().cpu().numpy() if _is_torch(freqs) else freqs, np.float64)
        if fr.ndim != 1 or fr.shape[0] != n_bins:
            raise ValueError(f"freqs must hold one entry per spectrum bin ({n_bins}), got shape {fr.shape}")
        if self._freqs is None or self._freqs.shape != fr.shape or not np.array_equal(self._freqs, fr):
            cfg = L.GenreConfig(int(self.sample_rate), int(n_bins))
            # (a refused table leaves the configured one, and with it the flux state, as it was)
            self._eng._check(L.lib().omega_genre_configure(self._eng._ctx, C.byref(cfg), fr.ctypes.data))
            self._freqs = fr.copy()
        return self._freqs

    def reset(self) -> None:
        """Forget the previous magnitude (the next frame's flux is 0)."""
        self._eng._check(L.lib().omega_genre_reset(self._eng._ctx))

    def extract_features_frames(self, spectra, freqs, frames):
        """spectra [F, K] float32, freqs [K], frames [F, m] float32 / float64 -- host numpy, or device torch
        tensors whose rows may overlap (an ``unfold`` view of a stream; a strided view of wider spectra).
        Returns (out [F, len(COLUMNS)] float64, peak_bins [F, 5] int32): numpy for host input, device
        tensors for device input. The frames are one stream in order: the flux of frame f compares with
        frame f-1, that of frame 0 with the last frame of the previous call."""
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
            pb = torch.empty((F, N_PEAKS), dtype=torch.int32, device=spectra.device)
            self._eng._bind_stream(spectra)
            self._eng._check(lib.omega_genre_features(
                self._eng._ctx, spectra.data_ptr(), spectra.stride(0) if F > 1 else K, frames.data_ptr(),
                int(frames.dtype == torch.float64), m, frames.stride(0) if F > 1 else m, F, out.data_ptr(),
                pb.data_ptr(), L.MEM_DEVICE))
            return out, pb
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
        pb = np.empty((F, N_PEAKS), np.int32)
        self._eng._check(lib.omega_genre_features(self._eng._ctx, spectra.ctypes.data, K, frames.ctypes.data,
                                                  int(frames.dtype == np.float64), m, m, F, out.ctypes.data,
                                                  pb.ctypes.data, L.MEM_HOST))
        return out, pb

    @staticmethod
    def _check_shape(K: int, m: int) -> None:
        # (both sizes are refused before either touches the configured table or the flux state)
        if not 16 <= K <= 8193:
            raise L.UnsupportedError(L.EUNSUP, f"genre: {K} spectrum bins (16..8193 are built)")
        if not 15 <= m <= 8192:
            raise L.UnsupportedError(L.EUNSUP, f"genre: {m} audio samples per frame (15..8192 are built)")

    # -- the reference's surface --
    def extract_features(self, fft_data, audio_chunk, freqs, drum_info: Dict, harmonic_info: Dict,
                         chromagram_data=None, chord_history: Optional[List[str]] = None,
                         key_history: Optional[List[str]] = None) -> Dict[str, float]:
        """:175-254 for one frame."""
        if len(fft_data) == 0 or len(audio_chunk) == 0:
            return {}
        out, _ = self.extract_features_frames(np.asarray(fft_data)[None, :], freqs, np.asarray(audio_chunk)[None, :])
        return self.features_from_row(out[0], len(audio_chunk), drum_info, harmonic_info, chromagram_data,
                                      chord_history, key_history)

    def features_from_row(self, row, n_samples: int, drum_info: Dict, harmonic_info: Dict, chromagram_data=None,
                          chord_history=None, key_history=None) -> Dict[str, float]:
        """The reference's feature dict from one device row and the host-side inputs."""
        v = {k: float(row[i]) for k, i in _COL.items()}
        features: Dict[str, float] = {}
        features["spectral_centroid"] = v["spectral_centroid"]
        features["spectral_rolloff"] = v["spectral_rolloff"]
        features["zero_crossing_rate"] = int(v["zero_crossings"]) / n_samples
        features["spectral_bandwidth"] = v["spectral_bandwidth"]
        features["dynamic_range"] = v["dynamic_range"]
        kick_mag = drum_info.get("kick", {}).get("magnitude", 0)
        snare_mag = drum_info.get("snare", {}).get("magnitude", 0)
        features["percussion_strength"] = max(kick_mag, snare_mag)
        series = harmonic_info.get("harmonic_series", [])
        if series and len(series) > 0:
            strengths = [h.get("strength", 0) for h in series if isinstance(h, dict)]
            if strengths:
                features["harmonic_complexity"] = min(1.0, (len(series) / 10.0) * np.mean(strengths))
            else:
                features["harmonic_complexity"] = min(1.0, len(series) / 10.0)
        else:
            features["harmonic_complexity"] = v["spectral_complexity"]
        features["estimated_tempo"] = self.estimate_tempo_from_transients(drum_info)
        if chromagram_data is not None and len(chromagram_data) == 12:
            chroma = np.asarray(chromagram_data)
            features["pitch_class_concentration"] = self.compute_pitch_class_concentration(chroma)
            features["pitch_class_entropy"] = self.compute_pitch_class_entropy(chroma)
        else:
            features["pitch_class_concentration"] = 0.5
            features["pitch_class_entropy"] = 0.5
        features["chord_change_rate"] = self.compute_chord_change_rate(chord_history) \
            if chord_history is not None and len(chord_history) > 1 else 0.0
        features["key_stability"] = self.compute_key_stability(key_history) \
            if key_history is not None and len(key_history) > 1 else 1.0
        features["bass_emphasis"] = v["bass_emphasis"]
        features["beat_regularity"] = self.compute_beat_regularity(drum_info)
        features["vocal_presence"] = v["vocal_presence"]
        features["high_freq_energy"] = v["high_freq_energy"]
        features["spectral_flux"] = v["spectral_flux"]
        score = 0.0
        for _ in range(int(v["distortion_count"])):  # (:315: added one by one)
            score += 0.2
        features["harmonic_distortion"] = min(score, 1.0)
        features["mid_frequency_dominance"] = v["mid_frequency_dominance"]
        features["power_chord_ratio"] = self.compute_power_chord_ratio(
            None if chromagram_data is None else np.asarray(chromagram_data))
        return features

    @staticmethod
    def estimate_tempo_from_transients(drum_info: Dict) -> float:
        return 120 if drum_info.get("kick", {}).get("kick_detected", False) else 0

    @staticmethod
    def compute_beat_regularity(drum_info: Dict) -> float:
        kick = drum_info.get("kick", {}).get("magnitude", 0)
        snare = drum_info.get("snare", {}).get("magnitude", 0)
        if kick > 0.7 and snare > 0.5:
            return 0.9
        if kick > 0.5 or snare > 0.4:
            return 0.7
        return 0.3

    @staticmethod
    def compute_pitch_class_concentration(chromagram) -> float:
        """:645-656: the Gini coefficient of the normalised chroma."""
        if chromagram is None or np.sum(chromagram) == 0:
            return 0.5
        s = np.sort(chromagram / np.sum(chromagram))
        n = len(s)
        return (2 * np.sum(np.arange(1, n + 1) * s)) / (n * np.sum(s)) - (n + 1) / n

    @staticmethod
    def compute_pitch_class_entropy(chromagram) -> float:
        if chromagram is None or np.sum(chromagram) == 0:
            return 0.0
        probs = chromagram / np.sum(chromagram)
        return -np.sum(probs * np.log2(probs + 1e-10)) / np.log2(12)

    @staticmethod
    def compute_chord_change_rate(chord_history: List[str]) -> float:
        if len(chord_history) < 2:
            return 0.0
        changes = sum(1 for i in range(1, len(chord_history)) if chord_history[i] != chord_history[i - 1])
        return changes / (len(chord_history) - 1)

    @staticmethod
    def compute_key_stability(key_history: List[str]) -> float:
        if len(key_history) < 2:
            return 1.0
        changes = sum(1 for i in range(1, len(key_history)) if key_history[i] != key_history[i - 1])
        return 1.0 - (changes / (len(key_history) - 1))

    @staticmethod
    def compute_power_chord_ratio(chromagram) -> float:
        """:351-380: a strong root and fifth with weak thirds."""
        if chromagram is None or len(chromagram) != 12:
            return 0.0
        total = np.sum(chromagram)
        if total == 0:
            return 0.0
        c = chromagram / total
        best = 0.0
        for root in range(12):
            fifth = (root + 7) % 12
            if c[root] > 0.1 and c[fifth] > 0.05 and c[(root + 4) % 12] < 0.03 and c[(root + 3) % 12] < 0.03:
                if 0.3 < c[fifth] / c[root] < 0.8:
                    best = max(best, c[root] + c[fifth])
        return min(best * 2, 1.0)

    def classify(self, features: Dict[str, float], hip_hop_confidence: Optional[float] = None) -> Dict[str, float]:
        """:424-597. ``hip_hop_confidence`` stands where the reference's HipHopDetector result would."""
        if not self.genre_patterns:
            raise ValueError("classify needs the genre_patterns table: GenreClassifier(fs, genre_patterns=...)")
        get = features.get
        scores: Dict[str, float] = {}
        for genre, patterns in self.genre_patterns.items():
            if genre == "Hip-Hop" and hip_hop_confidence is not None:
                scores[genre] = hip_hop_confidence
                continue
            score, weight = 0.0, 0.0
            for name, rng in patterns.items():
                if name == "priority" or not isinstance(rng, (tuple, list)):
                    continue
                lo, hi = rng
                if name in features:
                    val = features[name]
                    if lo <= val <= hi:
                        score += 1.0
                    elif val < lo:
                        score += max(0, 1 - (lo - val) / max(lo, 0.1)) * 0.5
                    else:
                        score += max(0, 1 - (val - hi) / max(hi, 0.1)) * 0.5
                    weight += 1.0
            base = score / weight if weight > 0 else 0.0
            if genre == "Metal":
                n = 0
                for key, thr, gain in (("zero_crossing_rate", 0.20, 1.3), ("harmonic_distortion", 0.5, 1.4),
                                       ("mid_frequency_dominance", 0.6, 1.2), ("power_chord_ratio", 0.3, 1.3),
                                       ("spectral_flux", 0.4, 1.2)):
                    if get(key, 0) > thr:
                        n += 1
                        base *= gain
                if n >= 3:
                    base *= 1.5
            elif genre == "Electronic":
                for key, thr, gain in (("harmonic_distortion", 0.4, 0.3), ("zero_crossing_rate", 0.18, 0.4),
                                       ("power_chord_ratio", 0.3, 0.5)):
                    if get(key, 0) > thr:
                        base *= gain
            elif genre == "Rock":
                for key, thr, gain in (("harmonic_distortion", 0.3, 1.2), ("mid_frequency_dominance", 0.5, 1.1)):
                    if get(key, 0) > thr:
                        base *= gain
            elif genre == "Country":
                for key, thr, gain in (("harmonic_distortion", 0.3, 0.3), ("zero_crossing_rate", 0.15, 0.4)):
                    if get(key, 0) > thr:
                        base *= gain
            scores[genre] = base * patterns.get("priority", 1.0)
        self.genre_history.append(scores)
        smoothed = {g: np.mean([h.get(g, 0) for h in self.genre_history]) for g in self.genres}
        if max(smoothed.values()) > 0:
            ranked = sorted(smoothed.items(), key=lambda x: x[1], reverse=True)
            smoothed[ranked[0][0]] *= 3.0 if ranked[0][1] > ranked[1][1] * 1.1 else 2.0
        total = sum(smoothed.values())
        if not total > 0:
            return {"Unknown": 1.0}
        for g in smoothed:
            smoothed[g] /= total
        exp = {g: np.exp(smoothed[g] * 5.0) for g in smoothed}
        exp_total = sum(exp.values())
        for g in smoothed:
            smoothed[g] = exp[g] / exp_total
        top = max(smoothed.values())
        if top > 0.2:
            for g in smoothed:
                if smoothed[g] == top:
                    smoothed[g] = min(0.95, top * 2.0)
                    break
            total = sum(smoothed.values())
            for g in smoothed:
                smoothed[g] /= total
        return smoothed

    @staticmethod
    def get_top_genres(probabilities: Dict[str, float], top_n: int = 3) -> List[Tuple[str, float]]:
        return sorted(probabilities.items(), key=lambda x: x[1], reverse=True)[:top_n]
