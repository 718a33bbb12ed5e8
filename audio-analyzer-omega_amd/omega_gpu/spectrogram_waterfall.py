"""The spectrogram waterfall on the MI355X: SpectrogramWaterfall and SpectrogramWaterfallPanel
(omega4/panels/spectrogram_waterfall.py) over libomega.so's omega_waterfall_rows and omega_waterfall_colors.

    p = SpectrogramWaterfallPanel(48000)
    p.update(fft_data, frequencies)          # what the main loop feeds the panel
    p.waterfall.update_batch(spectra)        # [F, n] consecutive frames in one call
    p.waterfall.get_image()                  # uint8 [rows, cells, 3] of the history in the current scheme
    p.get_results()                          # {'peak_freq', 'peak_magnitude', ...}

The device computes, per frame, the dB row of the displayed slice, its maximum and minimum, the 95th / 5th
percentile range over the last 20 frames, the normalised row and its RGB bytes, all in the spectrum's precision as
numpy runs the reference (float32 in, float32 rows; float64 in, float64 rows; anything else is widened to float64).
The state (20 maxima and minima, the current peak and floor) is a blob of float64 values that this object carries
from call to call; the library keeps nothing. include/omega.h has the definitions.

Differences from the reference:
  - a frame with a non-finite bin is skipped and logged: no row, no history entry, nothing changes;
  - a stream that changes precision must call reset() first (the library refuses the other precision's state);
  - nothing is drawn: draw() is replaced by get_image(); set_fonts() is accepted.
get_image() pads rows shorter than the longest with black (the reference leaves those pixels undrawn). Colours are
kept per row as the device wrote them and are made again, one omega_waterfall_colors call per run of rows of equal
length and type, when the scheme has changed.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from collections import deque
from typing import Any, Dict, List, Tuple

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _is_torch, _ptr
from .engine import utility_engine

log = logging.getLogger(__name__)

COLS = 7  # flags, dB max, dB min, peak, floor, argmax index, argmax value
FLAG_NONFINITE = 1
MAX_BINS = 8193
STATE_LEN = 45
SCHEMES = ['spectrum', 'hot', 'cool', 'viridis']
GREY = 4


def scheme_id(name) -> int:
    return SCHEMES.index(name) if name in SCHEMES else GREY


def frequency_mapping(sample_rate, fft_size, min_freq, max_freq) -> Tuple[int, int]:
    """_setup_frequency_mapping's (min_idx, max_idx) (:56-69) from the library; needs no device."""
    idx = (C.c_int32 * 2)()
    base = C.addressof(idx)
    L.check_plain(L.lib().omega_waterfall_mapping(float(sample_rate), int(fft_size), float(min_freq), float(max_freq),
                                                  base, base + C.sizeof(C.c_int32)),
                  "omega_waterfall_mapping: bad sample rate, transform size or frequency")
    return int(idx[0]), int(idx[1])


class SpectrogramWaterfall:
    def __init__(self, sample_rate: int = 48000, fft_size: int = 2048, device: int = 0):
        self._host_init(sample_rate, fft_size)
        self._eng = utility_engine(sample_rate, device)
        assert L.lib().omega_waterfall_state_size() == STATE_LEN

    def _host_init(self, sample_rate: int = 48000, fft_size: int = 2048) -> None:
        """The state that needs no device (the tests drive the host logic on it alone): :18-54."""
        self.sample_rate = sample_rate
        self.fft_size = fft_size
        self.waterfall_height = 200
        self.waterfall_data = deque(maxlen=self.waterfall_height)
        self.min_freq = 20
        self.max_freq = 20000
        self.freq_scale = 'log'
        self.dynamic_range = 80
        self.color_scheme = 'spectrum'
        self.auto_gain = True
        self.gain_adjustment = 0.0
        self.peak_history = deque(maxlen=100)
        self.current_peak = 0.0
        self.current_floor = -80.0
        self.freq_bins = None
        self.freq_indices = None
        self.show_frequency_grid = True
        self.show_time_grid = False
        self.grid_color = (80, 80, 100)
        self.update_counter = 0
        self.update_interval = 1
        self.skipped_nonfinite = 0
        self._state = None  # the device's blob (omega_waterfall_rows)
        self._colors = deque(maxlen=self.waterfall_height)  # (scheme id, uint8 [cells, 3]) beside each row
        self._configured = None
        self._last_argmax = None  # (index, value) of the newest frame that was processed
        self._eng = None
        self._setup_frequency_mapping()

    def _setup_frequency_mapping(self) -> None:
        """:56-69; the indices come from the library."""
        self.freq_bins = np.linspace(0, self.sample_rate / 2, self.fft_size // 2 + 1)
        lo, hi = frequency_mapping(self.sample_rate, self.fft_size, self.min_freq, self.max_freq)
        self.freq_indices = (lo, hi)
        self.display_freqs = self.freq_bins[lo:hi]

    # -- the device part --
    def _configure(self, n: int) -> Tuple[int, int]:
        lo, hi = self.freq_indices
        lo, hi = min(lo, n), min(hi, n)  # (Python's slice clamping on a shorter spectrum)
        if hi - lo < 1:
            raise ValueError(f"the spectrum's {n} bins leave the displayed slice [{lo}:{hi}] empty")
        if n > MAX_BINS:
            raise L.UnsupportedError(L.EUNSUP, f"waterfall: {n} bins per spectrum (1..{MAX_BINS} are built)")
        if self._configured != (n, lo, hi - lo):
            cfg = L.WaterfallConfig(n, lo, hi - lo)
            # (a refused shape leaves the configured one as it was)
            self._eng._check(L.lib().omega_waterfall_configure(self._eng._ctx, C.byref(cfg)))
            self._configured = (n, lo, hi - lo)
        return lo, hi - lo

    def analyze_frames(self, spectra, state=None, rgb: bool = True):
        """spectra [F, n] float32 / float64 (anything else is widened to float64), consecutive frames of one stream
        -- host numpy, or a device torch tensor whose rows may overlap. state: what an earlier call returned for the
        stream, or None for a new panel. Uses this object's auto_gain, gain_adjustment, color_scheme and range; nothing
        of this object changes. Returns (stats [F, 7] float64, rows [F, cells] in the input's type, rgb uint8 [F,
        cells, 3] or None, the new state): numpy for host input, device tensors for device input. F frames in one
        call equal F chained calls bit for bit."""
        dev = _is_torch(spectra)
        spectra, ptr, stride, f64 = M.rows(spectra, dev, "spectra must be [F, n]", audio=True)
        F, n = spectra.shape
        _, cells = self._configure(n)
        state = M.state_blob(state, spectra, STATE_LEN)
        stats = M.alloc(spectra, (F, COLS), np.float64)
        rows = M.alloc(spectra, (F, cells), np.float64 if f64 else np.float32)
        img = M.alloc(spectra, (F, cells, 3), np.uint8) if rgb else None
        new = M.alloc(spectra, (STATE_LEN,), np.float64)
        M.call(self._eng, L.lib().omega_waterfall_rows, spectra, ptr, stride, f64, F, int(bool(self.auto_gain)),
               float(self.gain_adjustment), scheme_id(self.color_scheme), _ptr(state), _ptr(new), _ptr(stats),
               _ptr(rows), _ptr(img))
        return stats, rows, img, new

    def colorize(self, intensity, scheme=None):
        """_spectrum_to_color (:142-205) over intensities [R, cells] (float32 or float64; host numpy or a device
        tensor) in `scheme` (a name; default: the current one) -> uint8 [R, cells, 3]."""
        dev = _is_torch(intensity)
        x, ptr, stride, f64 = M.rows(intensity, dev, "intensity must be [R, cells]", audio=True)
        R, K = x.shape
        out = M.alloc(x, (R, K, 3), np.uint8)
        M.call(self._eng, L.lib().omega_waterfall_colors, x, ptr, stride, f64, R, K,
               scheme_id(self.color_scheme if scheme is None else scheme), _ptr(out))
        return out

    def _rows(self, spectra):
        """The library call of update / update_batch on host frames [F, n] -> numpy (stats, rows, rgb, state)."""
        out = self.analyze_frames(spectra, self._state)
        return tuple(v.cpu().numpy() if _is_torch(v) else v for v in out)

    # -- the reference's surface --
    def update(self, fft_data, frequencies=None) -> None:
        """:71-106."""
        self.update_counter += 1
        if self.update_counter % self.update_interval != 0:
            return
        if fft_data is None or len(fft_data) == 0:
            return
        self._feed(fft_data[None, :] if _is_torch(fft_data) else np.asarray(fft_data)[None, :])

    def update_batch(self, spectra) -> None:
        """F consecutive frames [F, n] as F update() calls, in one library call: the frames update_interval lets
        through are picked on the host first."""
        if not _is_torch(spectra):
            spectra = np.asarray(spectra)
        F = len(spectra)
        keep =[i for i in range(F) if (self.update_counter + 1 + i) % self.update_interval == 0]
        self.update_counter += F
        if not keep or spectra.shape[1] == 0:
            return
        if len(keep) < F:
            spectra = spectra[keep]
        self._feed(spectra)

    def _feed(self, spectra) -> None:
        stats, rows, rgb, state = self._rows(spectra)
        sid = scheme_id(self.color_scheme)
        kind = rows.dtype.type
        for f in range(len(stats)):
            if int(stats[f, 0]) & FLAG_NONFINITE:
                self.skipped_nonfinite += 1
                log.warning("waterfall: a frame with a non-finite bin was skipped (%d so far)", self.skipped_nonfinite)
                continue
            self.peak_history.append((kind(stats[f, 1]), kind(stats[f, 2])))
            if self.auto_gain:
                self.current_peak, self.current_floor = kind(stats[f, 3]), kind(stats[f, 4])
            self.waterfall_data.append(rows[f].copy())
            self._colors.append((sid, rgb[f].copy()))
            self._last_argmax = (int(stats[f, 5]), kind(stats[f, 6]))
        self._state = state

    def get_image(self) -> np.ndarray:
        """uint8 [rows, cells, 3]: the history, oldest row first, in the current scheme (what the reference's
        _draw_waterfall paints cell by cell, without its scaling to pixels)."""
        data = list(self.waterfall_data)
        if not data:
            return np.zeros((0, 0, 3), np.uint8)
        sid = scheme_id(self.color_scheme)
        stale = [i for i, (s, _) in enumerate(self._colors) if s != sid]
        i = 0
        while i < len(stale):  # one call per run of adjacent stale rows of one length and type
            j = i
            while (j + 1 < len(stale) and stale[j + 1] == stale[j] + 1 and data[stale[j + 1]].shape == data[stale[i]].shape
                   and data[stale[j + 1]].dtype == data[stale[i]].dtype):
                j += 1
            img = self._colorize_rows(np.stack([data[k] for k in stale[i:j + 1]]), sid)
            for k, px in zip(stale[i:j + 1], img):
                self._colors[k] = (sid, px)
            i = j + 1
        width = max(len(r) for r in data)
        out = np.zeros((len(data), width, 3), np.uint8)
        for k, (_, px) in enumerate(self._colors):
            out[k, :len(px)] = px
        return out

    def _colorize_rows(self, rows, sid) -> np.ndarray:
        """The colours of stacked host rows [R, cells] in scheme id `sid` (the tests put a fake in its place)."""
        x, ptr, stride, f64 = M.rows(rows, False, "rows must be [R, cells]", audio=True)
        out = np.empty(x.shape + (3,), np.uint8)
        M.call(self._eng, L.lib().omega_waterfall_colors, x, ptr, stride, f64, x.shape[0], x.shape[1], sid, _ptr(out))
        return out

    def reset(self) -> None:
        """A new panel's state: the history, the range and the rows are dropped (needed before a stream changes
        precision)."""
        self._state = None
        self.peak_history.clear()
        self.current_peak = 0.0
        self.current_floor = -80.0
        self.clear_waterfall()
        self._last_argmax = None

    def _frequency_to_display_y(self, freq: float, display_height: int) -> int:
        """:123-140."""
        if self.freq_scale == 'log':
            lo = math.log10(max(self.min_freq, 1))
            hi = math.log10(self.max_freq)
            normalized = (math.log10(max(freq, 1)) - lo) / (hi - lo) if hi > lo else 0.0
        else:
            normalized = (freq - self.min_freq) / (self.max_freq - self.min_freq)
        return int(display_height * (1.0 - normalized))

    def get_frequency_labels(self, display_height: int) -> List[Tuple[float, int, str]]:
        """:207-230."""
        if self.freq_scale == 'log':
            marks = [20, 50, 100, 200, 500, 1000, 2000, 5000, 10000, 20000]
        else:
            marks = np.linspace(self.min_freq, self.max_freq, 10)
        labels = []
        for freq in marks:
            if not self.min_freq <= freq <= self.max_freq:
                continue
            if freq >= 1000:
                text = f"{freq/1000:.0f}k" if freq % 1000 == 0 else f"{freq/1000:.1f}k"
            else:
                text = f"{freq:.0f}"
            labels.append((freq, self._frequency_to_display_y(freq, display_height), text))
        return labels

    def set_color_scheme(self, scheme: str) -> None:
        if scheme in SCHEMES:
            self.color_scheme = scheme

    def set_frequency_range(self, min_freq: float, max_freq: float) -> None:
        """:237-241; the history and the state stay, as the reference's peak_history does."""
        self.min_freq = max(1, min_freq)
        self.max_freq = min(self.sample_rate / 2, max_freq)
        self._setup_frequency_mapping()

    def set_frequency_scale(self, scale: str) -> None:
        if scale in ['log', 'linear']:
            self.freq_scale = scale

    def adjust_gain(self, gain_db: float) -> None:
        self.gain_adjustment = gain_db

    def toggle_auto_gain(self) -> None:
        self.auto_gain = not self.auto_gain

    def clear_waterfall(self) -> None:
        self.waterfall_data.clear()
        self._colors.clear()


class SpectrogramWaterfallPanel:
    def __init__(self, sample_rate: int = 48000, device: int = 0):
        self._host_init(sample_rate)
        self.waterfall = SpectrogramWaterfall(sample_rate, device=device)

    def _host_init(self, sample_rate: int = 48000) -> None:
        """:264-286 without the waterfall (the tests put one on _host_init in its place)."""
        self.sample_rate = sample_rate
        self.waterfall = None
        self.waterfall_info = {
            'peak_freq': 0.0,
            'peak_magnitude': 0.0,
            'frequency_range': (20, 20000),
            'dynamic_range': 80,
            'color_scheme': 'spectrum'
        }
        self.paused = False
        self.zoom_factor = 1.0
        self.scroll_offset = 0
        self.font_large = self.font_medium = self.font_small = self.font_tiny = None

    def set_fonts(self, fonts) -> None:
        """Accepted; nothing is drawn."""
        self.font_large = fonts.get('large')
        self.font_medium = fonts.get('medium')
        self.font_small = fonts.get('small')
        self.font_tiny = fonts.get('tiny')

    def update(self, fft_data, frequencies) -> None:
        """:295-305. The argmax comes with the frame's row from the device; a frame that update_interval keeps
        from the waterfall is searched on the host, as the reference does."""
        if self.paused or fft_data is None or len(fft_data) == 0:
            return
        w = self.waterfall
        w._last_argmax = None
        skipped = w.skipped_nonfinite
        w.update(fft_data, frequencies)
        if w.skipped_nonfinite != skipped:
            return
        if w._last_argmax is None:  # (not handed to the device)
            a = fft_data.cpu().numpy() if _is_torch(fft_data) else np.asarray(fft_data)
            if not np.all(np.isfinite(a)):
                return
            k = int(np.argmax(a))
            w._last_argmax = (k, a[k])
        peak_idx, value = w._last_argmax
        if peak_idx < len(frequencies):
            self.waterfall_info['peak_freq'] = frequencies[peak_idx]
            self.waterfall_info['peak_magnitude'] = value

    def get_image(self) -> np.ndarray:
        return self.waterfall.get_image()

    def toggle_pause(self) -> None:
        self.paused = not self.paused

    def cycle_color_scheme(self) -> None:
        nxt = SCHEMES[(SCHEMES.index(self.waterfall.color_scheme) + 1) % len(SCHEMES)]
        self.waterfall.set_color_scheme(nxt)
        self.waterfall_info['color_scheme'] = nxt

    def toggle_frequency_scale(self) -> None:
        self.waterfall.set_frequency_scale('linear' if self.waterfall.freq_scale == 'log' else 'log')

    def adjust_gain(self, delta_db: float) -> None:
        self.waterfall.adjust_gain(self.waterfall.gain_adjustment + delta_db)

    def reset_view(self) -> None:
        self.waterfall.set_frequency_range(20, 20000)
        self.waterfall.gain_adjustment = 0.0
        self.zoom_factor = 1.0
        self.scroll_offset = 0

    def get_results(self) -> Dict[str, Any]:
        return self.waterfall_info.copy()
