"""Beat detection on the MI355X: the analysis of BeatDetector and BeatDetectionPanel
(omega4/panels/beat_detection.py:15-295, :297-384, :571-573) over libomega.so's omega_rhythm_features, with the
detector's onset history, adaptive threshold, beat times, tempo clustering, rhythmic pattern measures and beat
phase kept on the host.

    bp = BeatDetectionPanel(48000)
    bp.update(fft_data, audio_chunk, frequencies)     # what the app feeds the panel
    bp.get_results()                                  # {'current_bpm', 'bpm_confidence', 'is_beat', ...}
    rows, state = bp.detector.analyze_frames(spectra, frames, frequencies, state)   # [F, len(COLUMNS)]

The device computes, per frame, the spectral flux against the stream's previous live spectrum, the spectrum's sum,
the kick band and the band energies, and the panel's silence gate (omega_gpu._rhythm.COLUMNS; include/omega.h has
the definitions). The flux reads the stream's state, a blob of float64 values that this object carries from call
to call; the library keeps nothing. The host applies the reference's expressions to one row at a time, in the
reference's order and types.

The sums come back as float64 sums of the float32 bins and are rounded to np.float32 once, where the reference
holds numpy's float32 pairwise sums; from there the reference's expressions run in the reference's types. The
onset strength is a float32 quotient kept as np.float32 in the deques (the stream's first is the Python float 0.0,
as in the reference), so np.mean, np.std and np.fft.fft take the reference's type path. tests/test_rhythm.py
derives what the one rounding costs. Spectra are taken as float32, as the app passes them.

This project's rule for a frame with a non-finite sample or bin: the call changes nothing. A gated frame (the
panel's rms < 0.001) resets beat_info as :340-349 does and leaves the detector alone. Every time read goes through
`clock`. Drawing, fonts and colours are not built. Shapes outside this build (fewer than 2 or more than 8193 bins,
more than 16384 samples per frame) raise UnsupportedError.
"""
from __future__ import annotations

import time
from collections import deque
from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np

from . import _rhythm as R
from ._rhythm import COLUMNS, FLAG_GATED, FLAG_NO_FLUX, FLAG_NONFINITE  # noqa: F401

ENERGY_BANDS = {'sub_bass': (20, 60), 'bass': (60, 250), 'low_mid': (250, 500), 'mid': (500, 2000),
                'high_mid': (2000, 4000), 'high': (4000, 8000)}
_NO_PATTERNS = {'regularity': 0.0, 'complexity': 0.0, 'syncopation': 0.0, 'groove_strength': 0.0}


class BeatDetector:
    def __init__(self, sample_rate: int = 48000, device: int = 0, clock: Callable[[], float] = time.time):
        self._host_init(sample_rate, clock)
        self._dev = R.RhythmFeatures(sample_rate, device)

    def _host_init(self, sample_rate: int = 48000, clock: Callable[[], float] = time.time) -> None:
        """The state that needs no device (the tests drive the host logic on it alone): :18-62."""
        self.sample_rate = sample_rate
        self.onset_threshold = 0.3
        self.min_bpm = 60
        self.max_bpm = 200
        self.bpm_smoothing = 0.8
        self.onset_strength_history = deque(maxlen=100)
        self.peak_pick_threshold = 0.5
        self.peak_pick_delta = 0.1
        self.beat_times = deque(maxlen=32)
        self.current_bpm = 120.0
        self.bpm_confidence = 0.0
        self.beat_phase = 0.0
        self.tempo_candidates = {}
        self.tempo_history = deque(maxlen=50)
        self.downbeat_confidence = 0.0
        self.time_signature = (4, 4)
        self.rhythmic_complexity = 0.0
        self.energy_bands = dict(ENERGY_BANDS)
        self.energy_history = {band: deque(maxlen=20) for band in self.energy_bands}
        self.beat_strength = 0.0
        self.beat_regularity = 0.0
        self.syncopation_level = 0.0
        self._clock = clock
        self._state = None  # the device's stream state (omega_rhythm_features' blob): the reference's prev_spectrum

    @property
    def prev_spectrum(self):
        """The last live frame's spectrum (float32), or None at a stream's start."""
        if self._state is None:
            return None
        s = self._state.cpu().numpy() if R._is_torch(self._state) else self._state
        return s[2:].astype(np.float32) if s[0] else None

    def reset(self) -> None:
        """Back to the state of a new detector (the device keeps none)."""
        self._host_init(self.sample_rate, self._clock)

    # -- the device part --
    def analyze_frames(self, spectra, frames, frequencies, state=None):
        """spectra [F, K] float32, frames [F, m] float32 / float64 (or None: no gate) and the K frequencies,
        consecutive frames of one stream -- host numpy, or device torch tensors whose rows may overlap. state: what
        an earlier call returned for the stream, or None at its start. Returns ([F, len(COLUMNS)] float64, the new
        state). Nothing of this object changes; F frames in one call equal F chained calls bit for bit."""
        return self._dev.analyze_frames(spectra, frames, frequencies, state)

    # -- the host part --
    def _apply_row(self, row) -> Optional[Dict[str, Any]]:
        """BeatDetectionPanel.update()'s analysis (:351-363) from one device row: detect_beats, calculate_bpm,
        analyze_rhythmic_patterns and get_beat_phase in that order. None where the row was non-finite or gated:
        nothing changed."""
        flags = int(row[0])
        if flags & (FLAG_NONFINITE | FLAG_GATED):
            return None
        is_beat, beat_strength = self._detect_beats(row, flags)
        current_bpm, bpm_confidence = self.calculate_bpm()
        rhythmic_patterns = self.analyze_rhythmic_patterns()
        beat_phase = self.get_beat_phase()
        return {'current_bpm': current_bpm, 'bpm_confidence': bpm_confidence, 'is_beat': is_beat,
                'beat_strength': beat_strength, 'beat_phase': beat_phase, 'rhythmic_patterns': rhythmic_patterns,
                'last_beat_time': self.beat_times[-1] if self.beat_times else 0.0}

    def _detect_beats(self, row, flags: int) -> Tuple[bool, Any]:
        """:95-152. The reference's np.sum over the float32 spectrum is float32: the device's float64 sums are
        rounded to it once."""
        current_time = self._clock()
        for b, band_name in enumerate(self.energy_bands):  # :81-93
            self.energy_history[band_name].append(np.float32(row[5 + b]))
        spectral_energy = np.float32(row[2])
        if flags & FLAG_NO_FLUX:  # :66-68
            onset_strength = 0.0
        else:
            flux = np.float32(row[3])
            if spectral_energy > 0:
                flux = flux / spectral_energy
            onset_strength = flux
        self.onset_strength_history.append(onset_strength)
        is_beat = False
        beat_strength = 0.0
        if len(self.onset_strength_history) > 10:
            recent_onsets = list(self.onset_strength_history)[-10:]
            mean_onset = np.mean(recent_onsets)
            std_onset = np.std(recent_onsets)
            threshold = mean_onset + (self.onset_threshold * std_onset)
            if (onset_strength > threshold and
                    onset_strength > self.peak_pick_threshold):
                bass_energy = np.mean(list(self.energy_history['bass'])[-3:]) if self.energy_history['bass'] else 0
                kick_energy = np.float32(row[4])  # :140-152
                kick_strength = kick_energy / spectral_energy if spectral_energy > 0 else 0.0
                beat_strength = (onset_strength * 0.6 +
                                 bass_energy * 0.3 +
                                 kick_strength * 0.1)
                if not self.beat_times or (current_time - self.beat_times[-1]) > 0.2:
                    is_beat = True
                    self.beat_times.append(current_time)
                    self.beat_strength = beat_strength
        return is_beat, beat_strength

    def calculate_bpm(self) -> Tuple[float, float]:
        """:154-209."""
        if len(self.beat_times) < 4:
            return self.current_bpm, 0.0
        intervals = []
        beat_list = list(self.beat_times)
        for i in range(1, len(beat_list)):
            interval = beat_list[i] - beat_list[i - 1]
            if 0.3 <= interval <= 1.0:
                intervals.append(interval)
        if not intervals:
            return self.current_bpm, 0.0
        bpms = [60.0 / interval for interval in intervals]
        bpm_candidates = {}
        for bpm in bpms:
            rounded_bpm = round(bpm * 2) / 2
            if rounded_bpm not in bpm_candidates:
                bpm_candidates[rounded_bpm] = []
            bpm_candidates[rounded_bpm].append(bpm)
        best_bpm = self.current_bpm
        best_confidence = 0.0
        for candidate_bpm, bpm_list in bpm_candidates.items():
            if len(bpm_list) >= 2:
                confidence = len(bpm_list) / len(bpms)
                variance = np.var(bpm_list)
                confidence *= max(0.1, 1.0 - variance / 100.0)
                if confidence > best_confidence:
                    best_bpm = np.mean(bpm_list)
                    best_confidence = confidence
        if best_confidence > 0.3:
            self.current_bpm = (self.bpm_smoothing * self.current_bpm +
                                (1 - self.bpm_smoothing) * best_bpm)
            self.bpm_confidence = best_confidence
        self.tempo_history.append((self.current_bpm, self.bpm_confidence))
        return self.current_bpm, self.bpm_confidence

    def analyze_rhythmic_patterns(self) -> Dict[str, float]:
        """:211-258."""
        if len(self.beat_times) < 8:
            return dict(_NO_PATTERNS)
        intervals = []
        beat_list = list(self.beat_times)[-8:]
        for i in range(1, len(beat_list)):
            intervals.append(beat_list[i] - beat_list[i - 1])
        if intervals:
            mean_interval = np.mean(intervals)
            interval_variance = np.var(intervals)
            regularity = max(0.0, 1.0 - (interval_variance / (mean_interval ** 2)))
            self.beat_regularity = regularity
        if len(self.onset_strength_history) > 20:
            onset_array = np.array(list(self.onset_strength_history)[-20:])
            onset_fft = np.abs(np.fft.fft(onset_array))
            with np.errstate(invalid="ignore"):  # (twenty zero onsets: 0 / 0, and min(1.0, nan) is 1.0 as in the reference)
                spectral_centroid = np.sum(onset_fft * np.arange(len(onset_fft))) / np.sum(onset_fft)
            self.rhythmic_complexity = min(1.0, spectral_centroid / len(onset_fft))
        if len(self.beat_times) >= 4:
            self.syncopation_level = self._calculate_syncopation()
        groove_strength = (self.beat_regularity * 0.4 +
                           self.rhythmic_complexity * 0.3 +
                           self.syncopation_level * 0.3)
        return {'regularity': self.beat_regularity, 'complexity': self.rhythmic_complexity,
                'syncopation': self.syncopation_level, 'groove_strength': groove_strength}

    def _calculate_syncopation(self) -> float:
        """:260-280."""
        if len(self.onset_strength_history) < 16:
            return 0.0
        onset_pattern = np.array(list(self.onset_strength_history)[-16:])
        beat_positions = [0, 4, 8, 12]
        off_beat_positions = [2, 6, 10, 14]
        beat_strength = np.mean([onset_pattern[pos] for pos in beat_positions if pos < len(onset_pattern)])
        off_beat_strength = np.mean([onset_pattern[pos] for pos in off_beat_positions if pos < len(onset_pattern)])
        if beat_strength > 0:
            syncopation = off_beat_strength / beat_strength
            return min(1.0, syncopation)
        return 0.0

    def get_beat_phase(self) -> float:
        """:282-294."""
        if len(self.beat_times) < 2 or self.current_bpm <= 0:
            return 0.0
        current_time = self._clock()
        last_beat = self.beat_times[-1]
        beat_duration = 60.0 / self.current_bpm
        time_since_beat = current_time - last_beat
        self.beat_phase = (time_since_beat / beat_duration) % 1.0
        return self.beat_phase


def _silent_info() -> Dict[str, Any]:
    return {'current_bpm': 120.0, 'bpm_confidence': 0.0, 'is_beat': False, 'beat_strength': 0.0, 'beat_phase': 0.0,
            'rhythmic_patterns': {}, 'last_beat_time': 0.0}


class BeatDetectionPanel:
    def __init__(self, sample_rate: int = 48000, device: int = 0, clock: Callable[[], float] = time.time):
        self._host_init(sample_rate, clock)
        self.detector._dev = R.RhythmFeatures(sample_rate, device)

    def _host_init(self, sample_rate: int = 48000, clock: Callable[[], float] = time.time) -> None:
        """:300-318 minus fonts; the detector without its device part."""
        self.sample_rate = sample_rate
        self.detector = BeatDetector.__new__(BeatDetector)
        self.detector._host_init(sample_rate, clock)
        self.beat_info = _silent_info()
        self.beat_flash_time = 0
        self.beat_flash_duration = 15
        self.bpm_history_display = deque(maxlen=100)

    def _apply_row(self, row) -> bool:
        """update()'s body (:337-383) from one device row. False where the row was non-finite: nothing changed."""
        flags = int(row[0])
        if flags & FLAG_NONFINITE:
            return False
        if flags & FLAG_GATED:
            self.beat_info = _silent_info()
            return True
        info = self.detector._apply_row(row)
        self.beat_info = info
        if info['is_beat']:
            self.beat_flash_time = self.beat_flash_duration
        elif self.beat_flash_time > 0:
            self.beat_flash_time -= 1
        self.bpm_history_display.append(info['current_bpm'])
        return True

    def update(self, fft_data, audio_chunk, frequencies) -> None:
        """:333-383. fft_data and audio_chunk: host numpy or device tensors."""
        if fft_data is None or len(fft_data) == 0 or audio_chunk is None:
            return
        d = self.detector
        row, new = d._dev.one_frame(fft_data, audio_chunk, frequencies, d._state)
        if self._apply_row(row):
            d._state = new  # (a gated frame hands the state through unchanged)

    def get_results(self) -> Dict[str, Any]:
        """:571-573."""
        return self.beat_info.copy()
