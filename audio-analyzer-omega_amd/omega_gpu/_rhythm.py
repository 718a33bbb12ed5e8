"""The device part that beat_detection.py and frequency_band_tracker.py share: libomega.so's omega_rhythm_features,
one pass over a frame's spectrum for both panels (COLUMNS; include/omega.h has the definitions), the stream's state
carried as a blob by the caller."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

COLUMNS = ("flags", "sumsq", "spec_sum", "flux", "kick", "band0", "band1", "band2", "band3", "band4", "band5",
           "band6", "spec_fsum", "spread_sum")
FLAG_NONFINITE, FLAG_GATED, FLAG_NO_FLUX = 1, 2, 4
EDGE_HZ = (20, 50, 60, 120, 250, 500, 2000, 4000, 8000, 20000)
_UPPER_ONLY = (3, 9)  # 120 and 20000 Hz are never a band's lower edge
BANDS = ((0, 2), (2, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9))  # the seven bands as pairs of edges
MAX_BINS, MAX_FRAME = 8193, 16384
TRACKER_FRAME = 1  # the frame length configured for calls without audio (it is not read)


def edges(frequencies) -> Tuple[int, ...]:
    """The reference's own expression per edge frequency, np.argmax(freqs >= f) (beat_detection.py:85-89, :143-147,
    frequency_band_tracker.py:118-122); len(freqs) where that gives 0 for an edge that is only ever an upper one.
    The library reads a band's upper edge 0 as len(freqs) wherever an edge serves both ways."""
    f = np.asarray(frequencies.detach().cpu().numpy() if _is_torch(frequencies) else frequencies)
    e = [int(np.argmax(f >= hz)) for hz in EDGE_HZ]
    for i in _UPPER_ONLY:
        if e[i] == 0:
            e[i] = len(f)
    return tuple(e)


def empty_bands(frequencies) -> Tuple[int, ...]:
    """The tracker's bands whose bin range is empty (frequency_band_tracker.py:118-126: low_idx >= high_idx after
    the upper index 0 has become len(freqs)); the library sums such a band to 0."""
    f = np.asarray(frequencies.detach().cpu().numpy() if _is_torch(frequencies) else frequencies)
    e = [int(np.argmax(f >= hz)) for hz in EDGE_HZ]
    return tuple(b for b, (i, j) in enumerate(BANDS) if e[i] >= (e[j] if e[j] else len(f)))


def state_len(n_bins: int) -> int:
    return 2 + int(n_bins)


class RhythmFeatures:
    """A utility engine with the rhythm entry points configured on demand."""

    def __init__(self, sample_rate, device: int = 0):
        self._eng = utility_engine(sample_rate, device)
        self._configured: Optional[Tuple[int, int, bytes]] = None
        assert L.lib().omega_rhythm_state_size(513) == state_len(513)

    @staticmethod
    def check_shape(K: int, m: int) -> None:
        # (every size is refused before any touches the configured shape)
        if not 2 <= K <= MAX_BINS:
            raise L.UnsupportedError(L.EUNSUP, f"rhythm: {K} spectrum bins (2..{MAX_BINS} are built)")
        if not 1 <= m <= MAX_FRAME:
            raise L.UnsupportedError(L.EUNSUP, f"rhythm: {m} audio samples per frame (1..{MAX_FRAME} are built)")

    def configure(self, K: int, m: int, frequencies) -> None:
        self.check_shape(K, m)
        f = frequencies.detach().cpu().numpy() if _is_torch(frequencies) else frequencies
        f = np.ascontiguousarray(f, np.float64)
        if f.shape != (K,):
            raise ValueError("frequencies must hold one value per spectrum bin")
        key = (K, m, f.tobytes())
        if self._configured != key:
            cfg = L.RhythmConfig(int(K), int(m))
            e = np.asarray(edges(f), np.int32)
            # (a refused shape leaves the configured one as it was)
            self._eng._check(L.lib().omega_rhythm_configure(self._eng._ctx, C.byref(cfg), f.ctypes.data, e.ctypes.data))
            self._configured = key

    def analyze_frames(self, spectra, frames, frequencies, state=None):
        """spectra [F, K] float32 and frames [F, m] float32 / float64 (or None: no gate, sumsq 0), consecutive
        frames of one stream -- host numpy, or device torch tensors whose rows may overlap or be strided.
        frequencies: K values. state: what an earlier call returned for the stream, or None at its start. Returns
        ([F, len(COLUMNS)] float64, the new state): numpy for host input, device tensors for device input. F frames
        in one call equal F chained calls bit for bit."""
        dev = _is_torch(spectra)
        if frames is not None and dev != _is_torch(frames):
            raise ValueError(M.MIXED_SIDES)
        spectra, spec_ptr, spec_stride, _ = M.rows(spectra, dev, M.SPECTRA_FRAMES)
        F, K = spectra.shape
        if frames is None:
            frame_ptr, frame_stride, f64, m = None, 0, 0, TRACKER_FRAME
        else:
            frames, frame_ptr, frame_stride, f64 = M.rows(frames, dev, M.SPECTRA_FRAMES, audio=True)
            if frames.shape[0] != F:
                raise ValueError(M.SPECTRA_FRAMES)
            m = frames.shape[1]
        self.configure(K, m, frequencies)
        n = state_len(K)
        state = M.state_blob(state, spectra, n)
        out = M.alloc(spectra, (F, len(COLUMNS)), np.float64)
        new = M.alloc(spectra, (n,), np.float64)
        M.call(self._eng, L.lib().omega_rhythm_features, spectra, spec_ptr, spec_stride, frame_ptr, f64, F,
               frame_stride, _ptr(state), _ptr(new), _ptr(out))
        return out, new

    def one_frame(self, spectrum, audio, frequencies, state):
        """(row as numpy, the new state beside the input) of a single frame."""
        if audio is not None and _is_torch(spectrum) != _is_torch(audio):
            to_np = lambda x: x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)  # noqa: E731
            spectrum, audio = to_np(spectrum), to_np(audio)
        if not _is_torch(spectrum):
            spectrum = np.asarray(spectrum)
            audio = None if audio is None else np.asarray(audio)
        rows, new = self.analyze_frames(spectrum[None, :], None if audio is None else audio[None, :], frequencies, state)
        return (rows[0].cpu().numpy() if _is_torch(rows) else rows[0]), new
