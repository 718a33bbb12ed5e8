"""Transient detection on the MI355X: the analysis of TransientDetectionPanel
(omega4/panels/transient_detection.py:11-381, :559-574) over libomega.so's omega_tdetect_features, with the panel's
state, thresholds, medians, histories, classification ladder and event list kept on the host.

    tp = TransientDetectionPanel(48000)
    tp.update(audio_windowed, spectrum)      # what omega4_main.py:1154-1156 feeds the panel
    tp.get_status()                          # {'detected', 'strength', 'type', 'attack_time', ...}
    rows, state = tp.analyze_frames(spectra, frames, state)   # [F, K] float32, [F, m] -> [F, len(COLUMNS)]

It is not omega_gpu.transient.TransientAnalyzer (analyzers/transient.py): only the Hilbert envelope is shared.

The device computes, for every frame and unconditionally, each frame-local quantity of update() -- the smoothed
Hilbert envelope's mean, peak, energy, the 512-point flux spectrum, the 1024-point pre-emphasised phase spectrum,
the order-4 high-pass filtfilt's energy, the attack / decay indices and the classification sums -- and the two
that compare a frame with the ones before it, the spectral flux and the phase-deviation novelty (COLUMNS;
include/omega.h has the definitions). Those two read the stream's state, a blob of float64 values that this
object carries from call to call; the library keeps nothing. The host applies the reference's expressions to
one row at a time, in the reference's order and types.

The spectrum's sums come back as float64 sums of the float32 bins and are rounded to float32 here, where the
reference holds numpy's float32 pairwise sums: the centroid and the band energies agree with the reference's to
the pairwise-summation bound (tests/test_transient_detection.py derives it), not bit for bit. Spectra are taken
as float32, as the app passes them.

update(audio, None) computes abs(rfft(audio * hanning)) with numpy on the host (the reference does so when it
classifies). That path is a convenience for callers without a spectrum, not the hot path.

This project's rule for a frame with a non-finite sample or bin: the call leaves the state untouched. Drawing,
fonts and colours are not built. Shapes outside this build (a frame that is not a power of two 256..8192, fewer
than 2 or more than 8193 bins, a rate below 8000 Hz) raise UnsupportedError.
"""
from __future__ import annotations

import ctypes as C
import time
from collections import deque
from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

COLUMNS = ("flags", "envelope", "peak", "energy", "flux_sum", "flux", "novelty", "mag_sum", "hf_energy",
           "sign_diff", "peak_idx", "start_idx", "end_idx", "spec_sum", "spec_fsum", "rolloff_idx",
           "band0", "band1", "band2", "band3", "guards")
FLAG_NONFINITE, FLAG_NO_HF, FLAG_NO_NOVELTY_SHAPE, FLAG_NO_FLUX, FLAG_NO_NOVELTY = 1, 2, 4, 8, 16
FLUX_BINS, PHASE_BINS = 128, 513
STATE_LEN = 4 + FLUX_BINS + 2 * PHASE_BINS


def band_indices(sample_rate, n_bins: int) -> Tuple[int, ...]:
    """np.searchsorted(freqs, [0, 100, 250, 2000, fs / 2]) of :248-252 for a spectrum length, from the library."""
    r = (C.c_int32 * 5)()
    L.check_plain(L.lib().omega_tdetect_band_indices(float(sample_rate), int(n_bins), r),
                  "omega_tdetect_band_indices: bad sample rate or bin count")
    return tuple(int(v) for v in r)


class TransientDetectionPanel:
    def __init__(self, sample_rate, device: int = 0, clock: Callable[[], float] = time.time):
        self._host_init(sample_rate, clock)
        self._eng = utility_engine(sample_rate, device)
        assert L.lib().omega_tdetect_state_size() == STATE_LEN

    def _host_init(self, sample_rate, clock: Callable[[], float] = time.time) -> None:
        """The state that needs no device (the tests drive the host logic on it alone): :14-73 minus drawing."""
        self.sample_rate = sample_rate
        self.is_frozen = False
        self.transient_detected = False
        self.transient_strength = 0.0
        self.transient_history = deque(maxlen=300)
        self.attack_time = 0.0
        self.decay_time = 0.0
        self.transient_type = "None"
        self.peak_level = 0.0
        self.rms_level = 0.0
        self.crest_factor = 0.0
        self.dynamic_range = 0.0
        self.envelope = 0.0
        self.envelope_history = deque(maxlen=300)
        self.transient_events = deque(maxlen=50)
        self.last_transient_time = 0
        self.band_energies = np.zeros(4)
        self.update_counter = 0
        self.update_interval = 1
        self.sensitivity = 1.5
        self.prev_envelope = 0.0
        self.attack_threshold = 0.1
        self.spectral_flux_history = deque(maxlen=10)
        self.prev_phase = None
        self.prev_prev_phase = None
        self.novelty_history = deque(maxlen=50)
        self.last_centroid = 0.0
        self.last_zcr = 0.0
        self.last_rolloff = 0.0
        self._clock = clock
        self._flux_sums = deque(maxlen=10)  # np.sum(s) of each spectrum in spectral_flux_history (column 4)
        self._state = None                  # the device's stream state (omega_tdetect_features' blob)
        self._configured: Optional[Tuple[int, int]] = None

    def reset(self) -> None:
        """Back to the state of a new panel (the device keeps none)."""
        configured = self._configured
        self._host_init(self.sample_rate, self._clock)
        self._configured = configured

    # -- the device part --
    def _check_shape(self, K: int, m: int) -> None:
        # (every size is refused before any touches the configured shape)
        if not 2 <= K <= 8193:
            raise L.UnsupportedError(L.EUNSUP, f"tdetect: {K} spectrum bins (2..8193 are built)")
        if not (256 <= m <= 8192 and m & (m - 1) == 0):
            raise L.UnsupportedError(L.EUNSUP, f"tdetect: {m} audio samples per frame (the powers of two "
                                               "256..8192 are built)")
        if not self.sample_rate >= 8000:
            raise L.UnsupportedError(L.EUNSUP, f"tdetect: {self.sample_rate} Hz (8000 Hz and above are built)")

    def _configure(self, K: int, m: int) -> None:
        self._check_shape(K, m)
        if self._configured != (K, m):
            cfg = L.TdetectConfig(float(self.sample_rate), int(K), int(m))
            # (a refused shape leaves the configured one as it was)
            self._eng._check(L.lib().omega_tdetect_configure(self._eng._ctx, C.byref(cfg)))
            self._configured = (K, m)

    def analyze_frames(self, spectra, frames, state=None):
        """spectra [F, K] float32 and frames [F, m] float32 / float64, consecutive frames of one stream -- host
        numpy, or device torch tensors whose rows may overlap (an ``unfold`` view of a stream; a strided view of
        wider spectra). state: what an earlier call returned for the stream, or None at its start. Returns
        ([F, len(COLUMNS)] float64, the new state): numpy for host input, device tensors for device input.
        Nothing of this object changes; F frames in one call equal F chained calls bit for bit."""
        dev = _is_torch(spectra)
        if dev and not _is_torch(frames):
            raise ValueError(M.MIXED_SIDES)
        spectra, spec_ptr, spec_stride, _ = M.rows(spectra, dev, M.SPECTRA_FRAMES)
        frames, frame_ptr, frame_stride, f64 = M.rows(frames, dev, M.SPECTRA_FRAMES, audio=True)
        if frames.shape[0] != spectra.shape[0]:
            raise ValueError(M.SPECTRA_FRAMES)
        F, K = spectra.shape
        self._configure(K, frames.shape[1])
        state = M.state_blob(state, spectra, STATE_LEN)
        out = M.alloc(spectra, (F, len(COLUMNS)), np.float64)
        new = M.alloc(spectra, (STATE_LEN,), np.float64)
        M.call(self._eng, L.lib().omega_tdetect_features, spectra, spec_ptr, spec_stride, frame_ptr, f64, F,
               frame_stride, _ptr(state), _ptr(new), _ptr(out))
        return out, new

    # -- the host part --
    def _apply_row(self, row, n_bins: int, frame_len: int, state=None) -> bool:
        """update()'s body (:88-118) from one device row (state: the blob that came back with it, for
        spectral_flux_history and the two phase attributes; None leaves them as they were). False where the row
        was non-finite: nothing changed."""
        flags = int(row[0])
        if flags & FLAG_NONFINITE:
            return False
        self.update_counter += 1
        m = int(frame_len)
        # :88-98
        self.envelope = np.float64(row[1])
        self.envelope_history.append(self.envelope)
        self.peak_level = np.float64(row[2])
        self.rms_level = np.sqrt(np.float64(row[3]) / m)
        if self.rms_level > 0:
            self.crest_factor = 20 * np.log10(self.peak_level / self.rms_level)
        self._detect_transient(row, flags, state)
        self.transient_history.append(self.transient_strength)
        if self.transient_detected:
            self._classify_transient(row, int(n_bins), m)
            self._measure_attack_decay(row, m)
            self.transient_events.append({
                'time': self._clock(),
                'type': self.transient_type,
                'strength': self.transient_strength,
                'attack': self.attack_time
            })
        return True

    def _detect_transient(self, row, flags: int, state) -> None:
        """:133-210."""
        if self.prev_envelope > 0:
            energy_ratio = self.envelope / self.prev_envelope
            if energy_ratio > self.sensitivity:
                self.transient_detected = True
                self.transient_strength = min(1.0, (energy_ratio - 1.0) / 2.0)
            else:
                self.transient_detected = False
                self.transient_strength *= 0.85
        # :150-183 (every built frame has 256 samples or more)
        if not flags & FLAG_NO_FLUX:
            flux = np.float64(row[5])
            avg_flux = np.mean(list(self._flux_sums))
            if avg_flux > 0 and flux > avg_flux * 1.8:
                self.transient_detected = True
                divisor = max(avg_flux * 3, 0.001)
                self.transient_strength = max(self.transient_strength, min(1.0, flux / divisor))
        self._flux_sums.append(np.float64(row[4]))
        if state is not None:
            self.spectral_flux_history.append(np.array(state[4:4 + FLUX_BINS], np.float64))
        # :315-365
        if not flags & FLAG_NO_NOVELTY_SHAPE:
            if not flags & FLAG_NO_NOVELTY:
                novelty = np.float64(row[6])
                self.novelty_history.append(novelty)
                threshold = np.median(list(self.novelty_history)) * 2.5
                if threshold <= 0:
                    threshold = 0.001
                if novelty > threshold:
                    self.transient_detected = True
                    self.transient_strength = min(1.0, novelty / (threshold * 3))
            if state is not None:
                self.prev_phase = np.array(state[4 + FLUX_BINS:4 + FLUX_BINS + PHASE_BINS], np.float64)
                self.prev_prev_phase = np.array(state[4 + FLUX_BINS + PHASE_BINS:], np.float64)
        self.prev_envelope = self.envelope
        # :190-207
        if not flags & FLAG_NO_HF:
            hf_energy = np.float64(row[8])
            total_energy = np.float64(row[3])
            if total_energy > 0:
                hf_ratio = hf_energy / total_energy
                if hf_ratio > 0.3:
                    self.transient_detected = True
                    self.transient_strength = max(self.transient_strength, hf_ratio)
        self._update_adaptive_sensitivity()

    def _update_adaptive_sensitivity(self) -> None:
        """:367-381."""
        if len(self.transient_events) >= 10:
            times = [e['time'] for e in self.transient_events]
            intervals = np.diff(times[-10:])
            if len(intervals) > 0:
                avg_interval = np.mean(intervals)
                if avg_interval < 0.2:
                    self.sensitivity = min(2.5, self.sensitivity + 0.1)
                elif avg_interval > 1.0:
                    self.sensitivity = max(1.2, self.sensitivity - 0.1)

    def _classify_transient(self, row, K: int, m: int) -> None:
        """:212-277. The reference's np.sum over the float32 spectrum is float32: the device's float64 sums are
        rounded to it."""
        d = 1 / self.sample_rate
        val = 1.0 / ((K - 1) * 2 * d)  # np.fft.rfftfreq: freqs[k] = k * val
        spec_sum = np.float32(row[13])
        if spec_sum > 0:
            self.last_centroid = np.float64(row[14]) / spec_sum
        else:
            self.last_centroid = 0
        self.last_zcr = np.float64(row[9]) / (2 * m)
        if spec_sum > 0:
            self.last_rolloff = np.float64(int(row[15]) * val)
        else:
            self.last_rolloff = 0
        guards = int(row[20])
        for i in range(4):
            if guards >> i & 1:
                self.band_energies[i] = np.float32(row[16 + i])
        total_energy = np.sum(self.band_energies)
        if total_energy > 0:
            self.band_energies /= total_energy
        if self.band_energies[0] > 0.7 and self.last_centroid < 150:
            self.transient_type = "Kick"
        elif self.band_energies[1] > 0.4 and self.last_centroid > 200 and self.last_centroid < 800:
            if self.last_zcr > 0.1:
                self.transient_type = "Snare"
            else:
                self.transient_type = "Tom"
        elif self.last_zcr > 0.3 and self.last_rolloff > 5000:
            self.transient_type = "HiHat"
        elif self.last_centroid > 1000 and self.band_energies[3] > 0.4:
            self.transient_type = "Cymbal"
        elif self.band_energies[2] > 0.5:
            self.transient_type = "Perc"
        else:
            self.transient_type = "Other"

    def _measure_attack_decay(self, row, m: int) -> None:
        """:279-313 (every built frame has 100 samples or more)."""
        peak_idx = np.int64(row[10])
        if peak_idx > 0:
            self.attack_time = (peak_idx - int(row[11])) * 1000 / self.sample_rate
        if peak_idx < m - 1:
            self.decay_time = (int(row[12]) - peak_idx) * 1000 / self.sample_rate

    # -- the reference's surface --
    def update(self, audio_data, spectrum=None) -> None:
        """:79-118. With spectrum=None the magnitude spectrum of the Hann-windowed frame is computed with numpy on
        the host -- a convenience, not the hot path."""
        if self.is_frozen or len(audio_data) == 0:
            return
        if (self.update_counter + 1) % self.update_interval != 0:
            self.update_counter += 1
            return
        if spectrum is None:
            a = audio_data.detach().cpu().numpy() if _is_torch(audio_data) else np.asarray(audio_data)
            spectrum = np.abs(np.fft.rfft(a * np.hanning(len(a))))
            audio_data = a
        if _is_torch(spectrum) != _is_torch(audio_data):
            to_np = lambda x: x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)  # noqa: E731
            spectrum, audio_data = to_np(spectrum), to_np(audio_data)
        rows, new = self.analyze_frames(spectrum[None, :], audio_data[None, :], self._state)
        if _is_torch(rows):
            row, host = rows[0].cpu().numpy(), new.cpu().numpy()
        else:
            row, host = rows[0], new
        if self._apply_row(row, len(spectrum), len(audio_data), host):
            self._state = new

    def get_status(self) -> Dict[str, Any]:
        """:559-574."""
        return {
            'detected': self.transient_detected,
            'strength': self.transient_strength,
            'type': self.transient_type,
            'attack_time': self.attack_time,
            'decay_time': self.decay_time,
            'crest_factor': self.crest_factor,
            'recent_events': list(self.transient_events),
            'sensitivity': self.sensitivity,
            'centroid': self.last_centroid,
            'zcr': self.last_zcr,
            'rolloff': self.last_rolloff,
            'band_energies': self.band_energies.tolist()
        }
