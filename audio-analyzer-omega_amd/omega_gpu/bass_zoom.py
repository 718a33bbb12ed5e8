"""The bass zoom panel on the MI355X: the analysis of BassZoomPanel (omega4/panels/bass_zoom.py:15-232, :383-400)
over libomega.so's omega_basszoom_features.

    bz = BassZoomPanel(48000)
    bz.update(audio_data, drum_info)         # what the main loop feeds the panel
    bz.get_results()                         # {'bar_values', 'peak_values', 'freq_ranges', 'detail_bars'}
    rows, bars, peaks, peak_times, state = bz.analyze_frames(frames, times, state)   # [F, m], [F] -> per frame

The device computes, per frame, the Hann-windowed 8192-point spectrum's 20..200 Hz bins, the bar means, the
compensation, bass_max, the scale factor and the compressed values (ROW_HEAD columns, then one per bar), and then
runs the reference's float32 smoothing, clamp and peak hold over the call's frames in order (include/omega.h has
the definitions). The panel's state (bars, peaks, peak timestamps) is a blob of float64 values that this object
carries from call to call; the library keeps nothing.

The reference hands each frame to a worker thread through a queue of five and applies whatever result has
arrived, so which frames it processes depends on thread timing. There is no thread here: update() processes the
frame and applies the result at once, which is what the reference does when its worker keeps up. shutdown() is
kept and does nothing. ``clock`` stands in for time.time (the peak timestamps).

This project's rule for a frame with a non-finite sample: the call leaves every attribute and the state
untouched. A rate without a bin in 20..200 Hz gives the reference's one bar that never moves, on the host. Drawing
and fonts are not built. Rates with more than 256 bins in 20..200 Hz (below about 5760 Hz) and empty frames raise
UnsupportedError.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Any, Callable, Dict, Optional

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

ROW_HEAD = 3  # flags, bass_max, scale_factor
FLAG_NONFINITE = 1
MAX_BARS, MAX_BINS = 64, 256
STATE_LEN = 3 * MAX_BARS
FFT_SIZE = 8192


def bass_mapping(sample_rate):
    """setup_bass_mapping (:51-97) from the library: (freq_ranges, bin_mapping, compensation), or None where the
    rate has no bin in 20..200 Hz. UnsupportedError above the bin cap, OmegaError for a bad rate."""
    n = (C.c_int32 * 4)()
    ranges = np.zeros(2 * MAX_BARS, np.float64)
    comp = np.zeros(MAX_BARS, np.float64)
    i32 = C.sizeof(C.c_int32)
    base = C.addressof(n)
    code = L.lib().omega_basszoom_mapping(float(sample_rate), base, base + i32, base + 2 * i32, base + 3 * i32,
                                          ranges.ctypes.data, comp.ctypes.data)
    if code == L.EUNSUP:
        bins = np.fft.rfftfreq(FFT_SIZE, 1 / sample_rate)
        if not np.any((bins >= 20) & (bins <= 200)):
            return None
        raise L.UnsupportedError(code, f"basszoom: {sample_rate} Hz has more than {MAX_BINS} bins in 20..200 Hz")
    L.check_plain(code, "omega_basszoom_mapping: bad sample rate")
    bars, first, per, valid = (int(v) for v in n)
    freq_ranges = [(ranges[2 * i], ranges[2 * i + 1]) for i in range(bars)]
    mapping = [list(range(first + i * per, first + min((i + 1) * per, valid))) for i in range(bars)]
    return freq_ranges, mapping, comp[:bars].copy()


class BassZoomPanel:
    def __init__(self, sample_rate: int = 48000, clock: Callable[[], float] = time.time, device: int = 0):
        self._host_init(sample_rate, clock)
        self._eng = utility_engine(sample_rate, device)
        assert L.lib().omega_basszoom_state_size() == STATE_LEN

    def _host_init(self, sample_rate, clock: Callable[[], float] = time.time) -> None:
        """The state that needs no device (the tests drive the host logic on it alone): :18-44 minus the thread."""
        self.sample_rate = sample_rate
        self.bass_detail_bars = 64
        self.bass_bar_values = np.zeros(self.bass_detail_bars, dtype=np.float32)
        self.bass_peak_values = np.zeros(self.bass_detail_bars, dtype=np.float32)
        self.bass_peak_timestamps = np.zeros(self.bass_detail_bars, dtype=np.float64)
        self.bass_freq_ranges = []
        self.bass_bin_mapping = []
        self.latest_bass_result = None
        self.font_small = None
        self.font_tiny = None
        self.drum_info = {}
        self._clock = clock
        self._comp = np.zeros(0)
        self._state = None  # the device's blob (omega_basszoom_features)
        self._pending_state = None
        self._configured: Optional[int] = None
        self.setup_bass_mapping()

    def set_fonts(self, fonts) -> None:
        """Accepted; nothing is drawn."""
        self.font_small = fonts.get('small')
        self.font_tiny = fonts.get('tiny')

    def draw(self, *args, **kwargs) -> None:
        """Accepted; nothing is drawn."""

    def setup_bass_mapping(self) -> None:
        """:51-97."""
        m = bass_mapping(self.sample_rate)
        if m is None:  # :62-67 (the arrays keep their 64 entries, as in the reference)
            self.bass_freq_ranges = [(20, 200)]
            self.bass_bin_mapping = [[]]
            self.bass_detail_bars = 1
            return
        self.bass_freq_ranges, self.bass_bin_mapping, self._comp = m
        self.bass_detail_bars = len(self.bass_freq_ranges)
        self.bass_bar_values = np.zeros(self.bass_detail_bars, dtype=np.float32)
        self.bass_peak_values = np.zeros(self.bass_detail_bars, dtype=np.float32)
        self.bass_peak_timestamps = np.zeros(self.bass_detail_bars, dtype=np.float64)

    @property
    def _fallback(self) -> bool:
        return self.bass_detail_bars == 1 and self.bass_bin_mapping == [[]]

    # -- the device part --
    def _configure(self, m: int) -> None:
        if self._fallback:
            raise L.UnsupportedError(L.EUNSUP, f"basszoom: {self.sample_rate} Hz has no bin in 20..200 Hz")
        if m < 1:
            raise L.UnsupportedError(L.EUNSUP, "basszoom: an empty frame (1 sample and more are built)")
        if self._configured != m:
            cfg = L.BassZoomConfig(float(self.sample_rate), int(m))
            # (a refused shape leaves the configured one as it was)
            self._eng._check(L.lib().omega_basszoom_configure(self._eng._ctx, C.byref(cfg)))
            self._configured = m

    def analyze_frames(self, frames, times, state=None):
        """frames [F, m] float32 / float64, consecutive frames of one stream -- host numpy, or a device torch tensor
        whose rows may overlap (an ``unfold`` view of a stream). times [F]: each frame's time in seconds. state: what
        an earlier call returned for the stream, or None for a new panel. Returns (rows [F, ROW_HEAD + bars], bars,
        peaks, peak_times [F, bars] each, the new state), all float64: numpy for host input, device tensors for
        device input. Nothing of this object changes; F frames in one call equal F chained calls bit for bit."""
        nb = self.bass_detail_bars
        dev = _is_torch(frames)
        frames, frame_ptr, stride, f64 = M.rows(frames, dev, "frames must be [F, m]", audio=True)
        F, m = frames.shape
        self._configure(m)
        if dev:
            import torch
            times = torch.as_tensor(np.asarray(times, np.float64) if not _is_torch(times) else times,
                                    dtype=torch.float64, device=frames.device).contiguous()
        else:
            times = np.ascontiguousarray(times, np.float64)
        if (times.numel() if dev else times.size) != F:
            raise ValueError("times must hold one value per frame")
        state = M.state_blob(state, frames, STATE_LEN)
        rows = M.alloc(frames, (F, ROW_HEAD + nb), np.float64)
        bars, peaks, ptimes = (M.alloc(frames, (F, nb), np.float64) for _ in range(3))
        new = M.alloc(frames, (STATE_LEN,), np.float64)
        M.call(self._eng, L.lib().omega_basszoom_features, frames, frame_ptr, stride, f64, _ptr(times), F,
               _ptr(state), _ptr(rows), _ptr(bars), _ptr(peaks), _ptr(ptimes), _ptr(new))
        return rows, bars, peaks, ptimes, new

    # -- the host part --
    def _apply_row(self, row, now: float) -> bool:
        """The second pass of :198-226 from one device row at time ``now``, in the reference's expressions and
        numpy 2.x types; the result is applied at once. False where the row was non-finite: nothing changed."""
        if int(row[0]) & FLAG_NONFINITE:
            return False
        bar_values = self.bass_bar_values.copy()
        peak_values = self.bass_peak_values.copy()
        peak_timestamps = self.bass_peak_timestamps.copy()
        current_time = now
        for i in range(len(self.bass_bin_mapping)):
            if i >= len(bar_values) or len(self.bass_bin_mapping[i]) == 0:
                continue
            compressed_value = np.float64(row[ROW_HEAD + i])
            if compressed_value > bar_values[i]:
                bar_values[i] = bar_values[i] * 0.1 + compressed_value * 0.9
            else:
                bar_values[i] = bar_values[i] * 0.6 + compressed_value * 0.4
            bar_values[i] = max(0.0, min(1.0, bar_values[i]))
            if bar_values[i] > peak_values[i]:
                peak_values[i] = bar_values[i]
                peak_timestamps[i] = current_time
            elif current_time - peak_timestamps[i] > 3.0:
                peak_values[i] *= 0.95
        self.latest_bass_result = {'bar_values': bar_values, 'peak_values': peak_values,
                                   'peak_timestamps': peak_timestamps}
        self.apply_bass_results()
        return True

    # -- the reference's surface --
    def update(self, audio_data, drum_info: Dict = None) -> None:
        """:118-131, without the worker thread: the frame is processed and its result applied at once."""
        if not self._fallback:
            a = audio_data if _is_torch(audio_data) else np.asarray(audio_data)
            rows, bars, peaks, ptimes, new = self.analyze_frames(a[None, :], [self._clock()], self._state)
            if _is_torch(rows):
                rows, bars, peaks, ptimes = (v.cpu().numpy() for v in (rows, bars, peaks, ptimes))
            if not int(rows[0, 0]) & FLAG_NONFINITE:
                self.latest_bass_result = {'bar_values': bars[0].astype(np.float32),
                                           'peak_values': peaks[0].astype(np.float32),
                                           'peak_timestamps': ptimes[0].copy()}
                self._pending_state = new
        self.apply_bass_results()
        self.drum_info = drum_info if drum_info is not None else {}

    def apply_bass_results(self) -> None:
        """:133-139."""
        if self.latest_bass_result is not None:
            self.bass_bar_values = self.latest_bass_result['bar_values']
            self.bass_peak_values = self.latest_bass_result['peak_values']
            self.bass_peak_timestamps = self.latest_bass_result['peak_timestamps']
            self.latest_bass_result = None
            if self._pending_state is not None:
                self._state, self._pending_state = self._pending_state, None

    def get_results(self) -> Dict[str, Any]:
        """:383-390."""
        return {
            'bar_values': self.bass_bar_values.copy(),
            'peak_values': self.bass_peak_values.copy(),
            'freq_ranges': self.bass_freq_ranges.copy(),
            'detail_bars': self.bass_detail_bars
        }

    def shutdown(self) -> None:
        """:392-400: there is no thread to stop."""
