"""Frequency band energy tracking on the MI355X: the analysis of FrequencyBandTracker and
FrequencyBandTrackerPanel (omega4/panels/frequency_band_tracker.py:26-240, :242-303) over libomega.so's
omega_rhythm_features, with the 30-frame RMS, the peak hold and decay, the balance, the tilt and the
95th-percentile reference level kept on the host.

    tp = FrequencyBandTrackerPanel(48000)
    tp.update(fft_data, frequencies)          # what the app feeds the panel
    tp.get_results()                          # {'bands', 'dominant_band', 'spectral_centroid', ...}
    rows, state = tp.tracker.analyze_frames(spectra, frequencies)

The device computes, per frame, the seven band energies, the total, sum(freqs * s) and the spread's sum
(omega_gpu._rhythm.COLUMNS; columns 2, 5-11, 12 and 13 are read here; the call passes no audio, so no frame is
gated). The host applies the reference's expressions to one row at a time, in the reference's order and types: the
sums come back as float64 sums of the float32 bins and are rounded to np.float32 once, where the reference holds
numpy's float32 pairwise sums (tests/test_rhythm.py derives what that costs). The spread takes the device's centroid
(the float64 sum over the float32 total, as the reference divides), whose difference from the reference's enters
the spread at second order. Spectra are taken as float32.

This project's rule for a frame with a non-finite bin: the call changes nothing. Built for the seven default
bands: add_custom_band and remove_band raise UnsupportedError. Drawing, fonts and colours are not built.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass
from typing import Any, Dict, Tuple

import numpy as np

from . import _lib as L
from . import _rhythm as R
from ._rhythm import COLUMNS, FLAG_NONFINITE  # noqa: F401


@dataclass
class FrequencyBand:
    name: str
    low_freq: float
    high_freq: float
    color: Tuple[int, int, int]
    peak_hold: bool = True
    rms_window: int = 30


def _default_bands() -> Dict[str, FrequencyBand]:
    return {
        'sub_bass': FrequencyBand('Sub Bass', 20, 60, (150, 50, 200)),
        'bass': FrequencyBand('Bass', 60, 250, (200, 100, 100)),
        'low_mid': FrequencyBand('Low Mid', 250, 500, (200, 150, 100)),
        'mid': FrequencyBand('Mid', 500, 2000, (150, 200, 150)),
        'high_mid': FrequencyBand('High Mid', 2000, 4000, (100, 150, 200)),
        'presence': FrequencyBand('Presence', 4000, 8000, (100, 200, 250)),
        'brilliance': FrequencyBand('Brilliance', 8000, 20000, (200, 200, 250)),
    }


class FrequencyBandTracker:
    def __init__(self, sample_rate: int = 48000, device: int = 0):
        self._host_init(sample_rate)
        self._dev = R.RhythmFeatures(sample_rate, device)

    def _host_init(self, sample_rate: int = 48000) -> None:
        """The state that needs no device (the tests drive the host logic on it alone): :29-69."""
        self.sample_rate = sample_rate
        self.frequency_bands = _default_bands()
        self.band_energies = {}
        self.band_rms = {}
        self.band_peaks = {}
        self.band_history = {}
        self.peak_hold_duration = 90
        self.peak_decay_rate = 0.95
        for band_id in self.frequency_bands:
            self.band_energies[band_id] = 0.0
            self.band_rms[band_id] = 0.0
            self.band_peaks[band_id] = {'value': 0.0, 'hold_time': 0}
            self.band_history[band_id] = deque(maxlen=100)
        self.db_range = 60
        self.reference_level = 0.0
        self.auto_reference = True
        self.total_energy = 0.0
        self.spectral_centroid = 0.0
        self.spectral_spread = 0.0
        self.spectral_balance = {}
        self.__dict__.pop('total_energy_history', None)  # (:174: created by the first update)

    def reset(self) -> None:
        """Back to the state of a new tracker (the device keeps none)."""
        self._host_init(self.sample_rate)

    # -- the device part --
    def analyze_frames(self, spectra, frequencies):
        """spectra [F, K] float32 and the K frequencies -- host numpy, or device torch tensors whose rows may be
        strided. Returns [F, len(COLUMNS)] float64 beside the input (the flux column and the state serve the beat
        detector and are not kept). Nothing of this object changes."""
        return self._dev.analyze_frames(spectra, None, frequencies)[0]

    # -- the host part --
    def _apply_row(self, row, empty=()) -> bool:
        """update()'s body (:76-112) from one device row. empty: the bands whose bin range is empty for the
        frequencies in use (omega_gpu._rhythm.empty_bands): the reference gives those the Python float 0.0, not a
        float32 sum. False where the row was non-finite: nothing changed."""
        if int(row[0]) & FLAG_NONFINITE:
            return False
        self.total_energy = np.float32(row[2])
        if self.total_energy > 0:
            self.spectral_centroid = np.float64(row[12]) / self.total_energy
        for b, (band_id, band) in enumerate(self.frequency_bands.items()):
            energy = 0.0 if b in empty else np.float32(row[5 + b])  # :114-132
            self.band_energies[band_id] = energy
            self.band_history[band_id].append(energy)
            if len(self.band_history[band_id]) >= band.rms_window:
                recent_energies = list(self.band_history[band_id])[-band.rms_window:]
                self.band_rms[band_id] = np.sqrt(np.mean(np.array(recent_energies) ** 2))
            else:
                self.band_rms[band_id] = energy
            if band.peak_hold:
                self._update_peak_hold(band_id, energy)
        # :152-158 (the device formed the sum about its own centroid, the same quotient)
        if self.total_energy > 0 and self.spectral_centroid > 0:
            self.spectral_spread = np.sqrt(np.float64(row[13]) / self.total_energy)
        else:
            self.spectral_spread = 0.0
        self._calculate_spectral_balance()
        if self.auto_reference:
            self._update_reference_level()
        return True

    def _update_peak_hold(self, band_id: str, current_energy) -> None:
        """:134-150."""
        peak_info = self.band_peaks[band_id]
        if current_energy > peak_info['value']:
            peak_info['value'] = current_energy
            peak_info['hold_time'] = self.peak_hold_duration
        else:
            if peak_info['hold_time'] > 0:
                peak_info['hold_time'] -= 1
            else:
                peak_info['value'] *= self.peak_decay_rate
                peak_info['value'] = max(peak_info['value'], current_energy)

    def _calculate_spectral_balance(self) -> None:
        """:160-169."""
        total_rms = sum(self.band_rms.values())
        if total_rms > 0:
            for band_id in self.frequency_bands:
                self.spectral_balance[band_id] = self.band_rms[band_id] / total_rms
        else:
            for band_id in self.frequency_bands:
                self.spectral_balance[band_id] = 0.0

    def _update_reference_level(self) -> None:
        """:171-180, with its first call's quirk: the history is created then, and that call's total is the first
        entry."""
        if hasattr(self, 'total_energy_history'):
            if len(self.total_energy_history) >= 50:
                self.reference_level = np.percentile(list(self.total_energy_history), 95)
        else:
            self.total_energy_history = deque(maxlen=100)
        self.total_energy_history.append(self.total_energy)

    # -- the reference's surface --
    def update(self, fft_data, frequencies) -> None:
        """:71-112."""
        if fft_data is None or len(fft_data) == 0 or frequencies is None:
            return
        row, _ = self._dev.one_frame(fft_data, None, frequencies, None)
        self._apply_row(row, R.empty_bands(frequencies))

    def get_band_db(self, band_id: str, use_rms: bool = True) -> float:
        """:182-192."""
        if use_rms:
            energy = self.band_rms.get(band_id, 0.0)
        else:
            energy = self.band_energies.get(band_id, 0.0)
        if energy > 0 and self.reference_level > 0:
            return 20 * np.log10(energy / self.reference_level)
        else:
            return -60.0

    def get_band_normalized(self, band_id: str, use_rms: bool = True) -> float:
        """:194-199."""
        db_value = self.get_band_db(band_id, use_rms)
        normalized = (db_value + self.db_range) / self.db_range
        return max(0.0, min(1.0, normalized))

    def add_custom_band(self, band_id, name, low_freq, high_freq, color):
        raise L.UnsupportedError(L.EUNSUP, "band tracker: the seven default bands are built; custom bands are not")

    def remove_band(self, band_id):
        raise L.UnsupportedError(L.EUNSUP, "band tracker: the seven default bands are built; none can be removed")

    def get_dominant_band(self) -> Tuple[str, float]:
        """:219-225."""
        if not self.band_rms:
            return 'none', 0.0
        dominant_band = max(self.band_rms.items(), key=lambda x: x[1])
        return dominant_band

    def get_spectral_tilt(self) -> float:
        """:227-239."""
        high_freq_bands = ['high_mid', 'presence', 'brilliance']
        low_freq_bands = ['sub_bass', 'bass', 'low_mid']
        high_energy = sum(self.band_rms.get(band, 0.0) for band in high_freq_bands)
        low_energy = sum(self.band_rms.get(band, 0.0) for band in low_freq_bands)
        if low_energy > 0:
            return high_energy / low_energy
        else:
            return 0.0


class FrequencyBandTrackerPanel:
    def __init__(self, sample_rate: int = 48000, device: int = 0):
        self._host_init(sample_rate)
        self.tracker._dev = R.RhythmFeatures(sample_rate, device)

    def _host_init(self, sample_rate: int = 48000) -> None:
        """:245-263 minus fonts; the tracker without its device part."""
        self.sample_rate = sample_rate
        self.tracker = FrequencyBandTracker.__new__(FrequencyBandTracker)
        self.tracker._host_init(sample_rate)
        self.band_info = {'bands': {}, 'dominant_band': 'none', 'spectral_centroid': 0.0, 'spectral_spread': 0.0,
                          'spectral_tilt': 0.0, 'total_energy_db': -60.0}
        self.show_peak_holds = True
        self.show_rms_values = True
        self.show_balance_chart = True
        self.meter_style = 'vertical'

    def _apply_row(self, row, empty=()) -> bool:
        """update()'s body (:280-303) from one device row (empty: as the tracker's). False where the row was
        non-finite: nothing changed."""
        t = self.tracker
        if not t._apply_row(row, empty):
            return False
        self.band_info = {
            'bands': {
                band_id: {
                    'name': band.name,
                    'energy': t.band_energies[band_id],
                    'rms': t.band_rms[band_id],
                    'peak': t.band_peaks[band_id]['value'],
                    'db_value': t.get_band_db(band_id),
                    'normalized': t.get_band_normalized(band_id),
                    'balance': t.spectral_balance.get(band_id, 0.0),
                    'color': band.color
                }
                for band_id, band in t.frequency_bands.items()
            },
            'dominant_band': t.get_dominant_band()[0],
            'spectral_centroid': t.spectral_centroid,
            'spectral_spread': t.spectral_spread,
            'spectral_tilt': t.get_spectral_tilt(),
            'total_energy_db': 20 * np.log10(max(t.total_energy, 1e-10))
        }
        return True

    def update(self, fft_data, frequencies) -> None:
        """:278-303. (The reference's tracker returns early where frequencies is None and the panel then rebuilds
        band_info from the unchanged tracker; here such a call is a no-op as a whole.)"""
        if fft_data is None or len(fft_data) == 0 or frequencies is None:
            return
        row, _ = self.tracker._dev.one_frame(fft_data, None, frequencies, None)
        self._apply_row(row, R.empty_bands(frequencies))

    def get_results(self) -> Dict[str, Any]:
        return self.band_info.copy()

    def analyze_frames(self, spectra, frequencies):
        return self.tracker.analyze_frames(spectra, frequencies)
