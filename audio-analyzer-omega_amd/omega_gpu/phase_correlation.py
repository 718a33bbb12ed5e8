"""Stereo phase correlation on the MI355X: the analysis of PhaseCorrelationPanel
(omega4/panels/phase_correlation.py:11-252, :934-941) over libomega.so's omega_phase_correlation, with the
panel's statistics, histories and goniometer persistence kept on the host.

    pc = PhaseCorrelation(48000, 2048)
    pc.update(left, right)          # one stereo frame of 2048 samples per channel
    pc.get_status()                 # {'correlation', 'stereo_width', 'balance', 'mono_compatible'}
    rows, points = pc.analyze_batch(left_frames, right_frames)   # [F, m] each; state advances in frame order

The device computes, per frame and in one workgroup: the overall correlation, stereo width, balance and both
RMS values, the ten per-band correlations of the Hann-windowed magnitude spectra, and the goniometer points
(COLUMNS; include/omega.h has the definitions). Nothing numeric runs on the host.

The one deliberate departure: the reference's update() receives a mono frame and fabricates its right channel
with np.random phase shifts and a slow balance wobble (:91-122). That is not reproduced. update(left, right)
analyses the two channels it is given; update(left) alone uses left for both.

Precision: everything is float64 whatever the input dtype (float32 is widened on load). The reference would
do the time-domain part in float32 for float32 arrays; parity is defined against the reference called on
float64 arrays, which is what the app passes (its audio_windowed is float64).

Frames shorter than 101 samples are ignored (:93). Errors are logged and leave the state unchanged. Sizes
outside this build (a frame that is not a power of two 64..8192) raise UnsupportedError from analyze_batch;
update logs them. export_phase_data, the display modes and all drawing are not built.
"""
from __future__ import annotations

import ctypes as C
import logging
from collections import deque
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

logger = logging.getLogger(__name__)

COLUMNS = ("correlation", "stereo_width", "balance", "rms_left", "rms_right", "flags", "band_mask") + tuple(
    f"band_{b}" for b in range(10))
N_BANDS, N_POINTS = 10, 128
FLAG_NONFINITE, FLAG_NO_ENERGY, FLAG_FLAT = 1, 2, 4
WARN_HIGH = "High correlation - check mono compatibility"
WARN_CANCEL = "Phase cancellation detected"


class PhaseCorrelation:
    def __init__(self, sample_rate: int = 48000, frame_size: int = 2048, device: int = 0):
        if not sample_rate > 0:
            raise ValueError("Sample rate must be positive")
        self._host_init(sample_rate, frame_size)
        self._eng = utility_engine(sample_rate, device)

    def _host_init(self, sample_rate, frame_size: int = 2048) -> None:
        """The state that needs no device (the tests drive the host logic on it alone)."""
        self.sample_rate = sample_rate
        self.frame_size = int(frame_size)
        self.is_frozen = False
        self.correlation = 0.0
        self.correlation_history = deque(maxlen=300)
        self.stereo_width = 0.0
        self.balance = 0.0
        self.freq_bands = N_BANDS
        self.band_correlations = np.zeros(self.freq_bands)
        # :67-76, and exactly these values go to the library (it does not recompute them)
        self.band_frequencies = np.logspace(np.log10(20), np.log10(min(20000, sample_rate / 2)), self.freq_bands + 1)
        self.gonio_persistence: List[Dict[str, Any]] = []
        self.gonio_decay_rate = 0.95
        self.gonio_max_frames = 30
        self.correlation_stats = {"min": 0.0, "max": 0.0, "avg": 0.0, "peak_hold_time": 0, "warnings": []}
        self._configured: Optional[int] = None

    # -- the device part --
    def _configure(self, m: int) -> None:
        if not (64 <= m <= 8192 and m & (m - 1) == 0):
            raise L.UnsupportedError(L.EUNSUP, f"phase: {m} samples per frame (the powers of two 64..8192 are built)")
        if self._configured != m:
            cfg = L.PhaseConfig(int(self.sample_rate), int(m))
            edges = np.ascontiguousarray(self.band_frequencies, np.float64)
            self._eng._check(L.lib().omega_phase_configure(self._eng._ctx, C.byref(cfg), edges.ctypes.data))
            self._configured = m

    def analyze_frames(self, left, right):
        """left, right [F, m] float32 / float64: host numpy, or device torch tensors whose rows may overlap and
        share one row stride (the two halves of a planar [F, 2, m] batch). Returns (rows [F, len(COLUMNS)],
        points [F, 128, 2]) float64, numpy for host input and device tensors for device input. No state.
        A device operand is copied when its own layout needs it (_marshal.rows); when the two row strides then
        differ, both are copied. (An operand that is usable in place is no longer copied merely because the
        other one was, as long as the strides agree.)"""
        dev = _is_torch(left)
        if dev:
            message = "left and right must both be [F, m] device tensors"
            if not _is_torch(right) or left.shape != right.shape:
                raise ValueError(message)
            left, _, stride, f64 = M.rows(left, True, message, audio=True)
            right, _, right_stride, _ = M.rows(right.to(left.dtype), True, message, audio=True)
            if left.shape[0] > 1 and stride != right_stride:  # (one row stride serves both, or both are copied)
                left, right, stride = left.contiguous(), right.contiguous(), left.shape[1]
        else:
            message = "left and right must both be [F, m]"
            left, right = np.asarray(left), np.asarray(right)
            if left.dtype != np.float32 or right.dtype != np.float32:
                left, right = np.asarray(left, np.float64), np.asarray(right, np.float64)
            left, _, stride, f64 = M.rows(left, False, message, audio=True)
            right = M.rows(right, False, message, audio=True)[0]
            if left.shape != right.shape:
                raise ValueError(message)
        F, m = left.shape
        self._configure(m)
        rows = M.alloc(left, (F, len(COLUMNS)), np.float64)
        pts = M.alloc(left, (F, N_POINTS, 2), np.float64)
        if F:
            M.call(self._eng, L.lib().omega_phase_correlation, left, _ptr(left), _ptr(right), f64, stride, F,
                   _ptr(rows), _ptr(pts))
        return rows, pts

    # -- the reference's surface --
    def analyze_batch(self, left, right):
        """analyze_frames, then the panel state advanced over the frames in order (:124-145 per frame)."""
        rows, pts = self.analyze_frames(left, right)
        m = left.shape[1]
        if m > 100 and not self.is_frozen:
            hr = rows.cpu().numpy() if _is_torch(rows) else rows
            hp = pts.cpu().numpy() if _is_torch(pts) else pts
            for r, p in zip(hr, hp):
                self._apply_row(r, p, m)
        return rows, pts

    def update(self, left, right=None) -> None:
        """:82-145 for one stereo frame; with right=None both channels are `left`."""
        if self.is_frozen:
            return
        try:
            if len(left) <= 100:
                return
            right = left if right is None else right
            if _is_torch(left):
                self.analyze_batch(left[None, :], right[None, :])
            else:
                self.analyze_batch(np.asarray(left)[None, :], np.asarray(right)[None, :])
        except Exception as e:  # (the facades' convention: log, leave the state as it was)
            logger.error("phase correlation update failed: %s", e)

    @staticmethod
    def n_points(m: int) -> int:
        step = max(1, m // 100)
        return -(-m // step)

    def _apply_row(self, row, points, m: int) -> None:
        """One device row and its points into the panel state (:124-145)."""
        flags = int(row[5])
        if flags & FLAG_NONFINITE:
            logger.error("phase correlation: non-finite input, frame ignored")
            return
        self.correlation = float(row[0])
        self.correlation_history.append(self.correlation)
        self.stereo_width = float(row[1])
        if not flags & FLAG_NO_ENERGY:
            self.balance = float(row[2])
        frame = [(float(x), float(y)) for x, y in points[:self.n_points(m)]]
        self.gonio_persistence.append({"points": frame, "intensity": 1.0})
        self.gonio_persistence = [{"points": f["points"], "intensity": f["intensity"] * self.gonio_decay_rate}
                                  for f in self.gonio_persistence if f["intensity"] > 0.1][-self.gonio_max_frames:]
        mask = int(row[6])
        for b in range(self.freq_bands):
            if mask >> b & 1:
                self.band_correlations[b] = row[7 + b]
        self._update_statistics()

    def _update_statistics(self) -> None:
        """:229-241."""
        if len(self.correlation_history) > 0:
            st = self.correlation_stats
            st["min"] = min(self.correlation_history)
            st["max"] = max(self.correlation_history)
            st["avg"] = np.mean(self.correlation_history)
            st["warnings"] = []
            if abs(st["avg"]) > 0.8:
                st["warnings"].append(WARN_HIGH)
            if self.correlation < -0.5:
                st["warnings"].append(WARN_CANCEL)

    def reset_statistics(self) -> None:
        """:243-252."""
        self.correlation_stats = {"min": 0.0, "max": 0.0, "avg": 0.0, "peak_hold_time": 0, "warnings": []}
        self.correlation_history.clear()

    def get_status(self) -> Dict[str, Any]:
        """:934-941."""
        return {"correlation": self.correlation, "stereo_width": self.stereo_width, "balance": self.balance,
                "mono_compatible": abs(self.correlation) < 0.8}
