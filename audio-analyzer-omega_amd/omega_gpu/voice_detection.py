"""Voice detection on the MI355X: the analysis of VoiceDetectionPanel
(omega4/panels/voice_detection.py:11-192, :299-307) over libomega.so's omega_voice_features, with the panel's
state, histories and scalar logic kept on the host.

    vp = VoiceDetectionPanel(48000)
    vp.update(audio_windowed, spectrum)      # what omega4_main.py:1147-1148 feeds the panel
    vp.get_status()                          # {'active', 'confidence', 'pitch', 'voice_type', 'formants'}
    rows = vp.analyze_frames(spectra, frames)   # [F, K] float32 and [F, m] -> [F, len(COLUMNS)]; no state

The device computes, per frame: the voice-band and total energy sums, the formant peaks (Savitzky-Golay
smoothing, scipy's find_peaks with its prominence rule, the first peak of each formant range) and the
autocorrelation's zero lag and best lag in the 80..400 Hz range (COLUMNS; include/omega.h has the
definitions). The host forms the ratio, the confidence, the decisions and the histories exactly as the
reference's expressions do, in the reference's types (np.float32 confidence, np.float64 pitch and formants).

The sums come back as float64 sums of the float32 bins and are rounded to float32 here, where the reference
holds numpy's float32 pairwise sums: the confidence agrees with the reference's to the pairwise-summation
bound (a few 1e-4 at the most, see tests/test_voice.py), not bit for bit.

update(audio, None) computes abs(rfft(audio * hanning)) with numpy on the host, as the reference does. That
path is a convenience for callers without a spectrum, not the hot path; the app always passes one.

This project's rule for a frame with a non-finite bin or sample: the call leaves the state untouched (the
reference would carry NaN into its confidence and histories). vocal_quality stays 0.0 as in the reference,
which never computes it. Drawing, fonts and colours are not built. Shapes outside this build (more than 8193
bins, a frame that is not a power of two 64..8192, a rate below 8000 Hz) raise UnsupportedError.
"""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

COLUMNS = ("flags", "voice_start", "voice_end", "voice_energy", "total_energy", "formant_count",
           "f1_bin", "f2_bin", "f3_bin", "f4_bin", "f1_freq", "f2_freq", "f3_freq", "f4_freq",
           "corr0", "peak_lag", "corr_peak")
FLAG_RANGE, FLAG_NO_ENERGY, FLAG_NONFINITE, FLAG_NO_PITCH = 1, 2, 4, 8


def voice_bin_range(sample_rate, frame_len: int) -> Tuple[int, int]:
    """(voice_start, voice_end) of :64-67 for a frame length, from the library (no device)."""
    r = (C.c_int32 * 2)()
    L.check_plain(L.lib().omega_voice_bin_range(float(sample_rate), int(frame_len), r),
                  "omega_voice_bin_range: bad sample rate or frame length")
    return int(r[0]), int(r[1])


class VoiceDetectionPanel:
    def __init__(self, sample_rate, device: int = 0):
        self._host_init(sample_rate)
        self._eng = utility_engine(sample_rate, device)

    def _host_init(self, sample_rate) -> None:
        """The state that needs no device (the tests drive the host logic on it alone): :14-51 minus drawing."""
        self.sample_rate = sample_rate
        self.is_frozen = False
        self.voice_active = False
        self.voice_confidence = 0.0
        self.voice_history = deque(maxlen=120)
        self.formants = []
        self.formant_history = deque(maxlen=60)
        self.voice_pitch = 0.0
        self.pitch_history = deque(maxlen=120)
        self.voice_type = "Unknown"
        self.vocal_quality = 0.0
        self.update_counter = 0
        self.update_interval = 2
        self._configured: Optional[Tuple[int, int]] = None

    def reset(self) -> None:
        """Back to the state of a new panel (the device keeps none)."""
        configured = self._configured
        self._host_init(self.sample_rate)
        self._configured = configured

    # -- the device part --
    def _check_shape(self, K: int, m: int) -> None:
        # (every size is refused before any touches the configured shape)
        if not 1 <= K <= 8193:
            raise L.UnsupportedError(L.EUNSUP, f"voice: {K} spectrum bins (1..8193 are built)")
        if not (64 <= m <= 8192 and m & (m - 1) == 0):
            raise L.UnsupportedError(L.EUNSUP, f"voice: {m} audio samples per frame (the powers of two 64..8192 "
                                               "are built)")
        if not self.sample_rate >= 8000:
            raise L.UnsupportedError(L.EUNSUP, f"voice: {self.sample_rate} Hz (8000 Hz and above are built)")

    def _configure(self, K: int, m: int) -> None:
        self._check_shape(K, m)
        if self._configured != (K, m):
            cfg = L.VoiceConfig(float(self.sample_rate), int(K), int(m))
            # (a refused shape leaves the configured one as it was)
            self._eng._check(L.lib().omega_voice_configure(self._eng._ctx, C.byref(cfg)))
            self._configured = (K, m)

    def analyze_frames(self, spectra, frames):
        """spectra [F, K] float32 and frames [F, m] float32 / float64 -- host numpy, or device torch tensors whose
        rows may overlap (an ``unfold`` view of a stream; a strided view of wider spectra). Returns
        [F, len(COLUMNS)] float64: numpy for host input, a device tensor for device input. The frames are
        independent and no state changes."""
        dev = _is_torch(spectra)
        if dev and not _is_torch(frames):
            raise ValueError(M.MIXED_SIDES)
        spectra, spec_ptr, spec_stride, _ = M.rows(spectra, dev, M.SPECTRA_FRAMES)
        frames, frame_ptr, frame_stride, f64 = M.rows(frames, dev, M.SPECTRA_FRAMES, audio=True)
        if frames.shape[0] != spectra.shape[0]:
            raise ValueError(M.SPECTRA_FRAMES)
        F, K = spectra.shape
        m = frames.shape[1]
        self._configure(K, m)
        out = M.alloc(spectra, (F, len(COLUMNS)), np.float64)
        if F:
            M.call(self._eng, L.lib().omega_voice_features, spectra, spec_ptr, spec_stride, frame_ptr, f64, m,
                   frame_stride, F, _ptr(out))
        return out

    def _row(self, audio_data, spectrum) -> np.ndarray:
        if _is_torch(spectrum) and _is_torch(audio_data):
            return self.analyze_frames(spectrum[None, :], audio_data[None, :])[0].cpu().numpy()
        to_np = lambda x: x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)  # noqa: E731
        return self.analyze_frames(to_np(spectrum)[None, :], to_np(audio_data)[None, :])[0]

    # -- the host part --
    def result_from_row(self, row, n_bins: Optional[int] = None) -> Dict[str, Any]:
        """One device row as the reference's values, no state changed (n_bins: the row's spectrum length, by
        default the configured one; it matters only at 10 bins and fewer). Keys: 'valid' (False: a
        non-finite input, nothing else is set); 'range_ok' (:69); with it 'active' and 'confidence' (:74-85) and
        'formants' (the list of :117, or None where the reference leaves its own as it was: a non-positive
        total, or n_bins <= 10); 'pitch' (:190-191, or None where it takes none)."""
        flags = int(row[0])
        if flags & FLAG_NONFINITE:
            return {"valid": False}
        if n_bins is None:
            n_bins = self._configured[0] if self._configured else 11
        res: Dict[str, Any] = {"valid": True, "range_ok": not flags & FLAG_RANGE, "formants": None, "pitch": None}
        if res["range_ok"]:
            if flags & FLAG_NO_ENERGY:
                res["active"], res["confidence"] = False, 0.0
            else:
                # the reference's sums are float32 (np.sum of float32 arrays), and so is everything after them
                voice_ratio = np.float32(row[3]) / np.float32(row[4])
                formant_score = 0.0
                if n_bins > 10:
                    res["formants"] = [np.float64(row[10 + r]) for r in range(4) if row[6 + r] > 0][:4]
                    formant_score = int(row[5]) / 4.0
                res["confidence"] = min(100, (voice_ratio * 200 + formant_score * 100) / 2)
                res["active"] = res["confidence"] > 30
        if not flags & FLAG_NO_PITCH and row[16] > 0.3 * row[14]:
            res["pitch"] = self.sample_rate / np.int64(row[15])
        return res

    def _apply_voice(self, res: Dict[str, Any]) -> None:
        if res["range_ok"]:  # (else :69 leaves the state as it was)
            if res["formants"] is not None:
                self.formants = res["formants"]
            self.voice_confidence = res["confidence"]
            self.voice_active = res["active"]

    def _apply_pitch(self, res: Dict[str, Any]) -> None:
        if res["pitch"] is not None:
            self.voice_pitch = res["pitch"]
            self.pitch_history.append(self.voice_pitch)

    def _apply_row(self, row, n_bins: int, has_audio: bool = True) -> bool:
        """update()'s body (:153-167) from one device row; False where the row was non-finite."""
        res = self.result_from_row(row, n_bins)
        if not res["valid"]:
            return False
        self._apply_voice(res)
        self.voice_history.append(self.voice_confidence)
        if self.voice_active and len(self.formants) > 0:
            self.formant_history.append(self.formants[:])
        if self.voice_active and has_audio:
            self._apply_pitch(res)
            self.analyze_voice_type()
        return True

    # -- the reference's surface --
    def detect_voice(self, audio_data, spectrum):
        """:57-87."""
        res = self.result_from_row(self._row(audio_data, spectrum), len(spectrum))
        if res["valid"]:
            self._apply_voice(res)
        return self.voice_active, self.voice_confidence

    def detect_pitch(self, audio_data) -> None:
        """:169-192."""
        if len(audio_data) < 2048:
            return
        one = np.ones(1, np.float32)
        if _is_torch(audio_data):
            import torch
            one = torch.ones(1, dtype=torch.float32, device=audio_data.device)
        res = self.result_from_row(self._row(audio_data, one), 1)
        if res["valid"]:
            self._apply_pitch(res)

    def analyze_voice_type(self) -> None:
        """:124-136."""
        if self.voice_pitch > 0:
            if self.voice_pitch < 110:
                self.voice_type = "Bass"
            elif self.voice_pitch < 165:
                self.voice_type = "Baritone"
            elif self.voice_pitch < 262:
                self.voice_type = "Tenor"
            elif self.voice_pitch < 330:
                self.voice_type = "Alto"
            else:
                self.voice_type = "Soprano"

    def update(self, audio_data, spectrum=None) -> None:
        """:138-167. With spectrum=None the magnitude spectrum of the Hann-windowed frame is computed with
        numpy on the host, as the reference does -- a convenience, not the hot path."""
        if self.is_frozen:
            return
        self.update_counter += 1
        if self.update_counter % self.update_interval != 0:
            return
        if spectrum is None and len(audio_data) > 0:
            a = audio_data.detach().cpu().numpy() if _is_torch(audio_data) else np.asarray(audio_data)
            spectrum = np.abs(np.fft.rfft(a * np.hanning(len(a))))
            audio_data = a
        if spectrum is not None and len(spectrum) > 0:
            if len(audio_data) > 0:
                self._apply_row(self._row(audio_data, spectrum), len(spectrum))

    def get_status(self) -> Dict[str, Any]:
        """:299-307."""
        return {
            "active": self.voice_active,
            "confidence": self.voice_confidence,
            "pitch": self.voice_pitch,
            "voice_type": self.voice_type,
            "formants": self.formants.copy() if self.formants else [],
        }
