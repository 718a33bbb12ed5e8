"""Drop-in ProfessionalMetering and ProfessionalMetersPanel over libomega.so
(omega4/panels/professional_meters.py:13-299 and :302-397, :516-579).

``calculate_lufs`` returns the same (mutated, shared) ``current_lufs`` dict with the same keys; the
K-weighting, the instantaneous LUFS, the 4x true peak and the momentary / short-term / integrated /
range / peak-hold deques all run on the MI355X (the deques live in the context as device-side
per-stream history). Filter coefficients are derived in the library (closed forms of
scipy.signal.butter / lfilter_zi) and exposed here for inspection.

Frames of any length are metered, like the reference (its 4800-sample chunks included): the weighting
runs scipy's float64 filtfilt cascade on the device (omega_weighting, any length above filtfilt's
padlen of 9), the true peak the polyphase form of scipy's resample on the power-of-two kernels or, for
other lengths, the mixed-radix transform (anyfft.hip). Nothing here raises to the caller (the
reference's convention): errors (e.g. a frame of 9 samples or fewer, where scipy's filtfilt raises)
are logged and the previous values (or, for the weighted signal, zeros) returned. calculate_true_peak
supports oversampling 1, 2 and 4 (the reference's default; 1 and 2 are phase subsets of the 4x form).
"""
from __future__ import annotations

import ctypes as C
import logging
from collections import deque
from typing import Any, Dict, Tuple

import numpy as np

from . import _lib as L
from . import _marshal as M
from ._marshal import _ptr
from .engine import utility_engine

logger = logging.getLogger(__name__)

def _butter2_highpass(fc: float, fs: float):
    k = np.tan(np.pi * fc / fs)
    n = 1 + np.sqrt(2) * k + k * k
    return np.array([1.0, -2.0, 1.0]) / n, np.array([1.0, 2 * (k * k - 1) / n, (1 - np.sqrt(2) * k + k * k) / n])


def _butter2_lowpass(fc: float, fs: float):
    k = np.tan(np.pi * fc / fs)
    n = 1 + np.sqrt(2) * k + k * k
    return np.array([k * k, 2 * k * k, k * k]) / n, np.array([1.0, 2 * (k * k - 1) / n, (1 - np.sqrt(2) * k + k * k) / n])


def _butter1(fc: float, fs: float, high: bool):
    k = np.tan(np.pi * fc / fs)
    b = np.array([1.0, -1.0]) / (1 + k) if high else np.array([k, k]) / (1 + k)
    return b, np.array([1.0, (k - 1) / (k + 1)])


class ProfessionalMetering:
    """Professional audio metering standards (LUFS, K-weighting, True Peak)."""

    def __init__(self, sample_rate: int = 48000, device: int = 0):
        self.sample_rate = sample_rate
        self.gate_threshold = -70.0
        self.weighting_mode = "K"
        self.k_weighting_filter = self.create_k_weighting_filter()
        self.current_lufs = {"momentary": -100.0, "short_term": -100.0, "integrated": -100.0, "range": 0.0,
                             "true_peak": -100.0}
        self.current_true_peak = -100.0
        self.a_weighting_filter = self.create_a_weighting_filter()
        self.c_weighting_filter = self.create_c_weighting_filter()
        # one context: its meter state is the four deques of :20-25 for one stream
        self._eng = utility_engine(sample_rate, device)

    @staticmethod
    def _frame(audio_data):
        return np.asarray(audio_data, dtype=np.float32).ravel()

    @staticmethod
    def _tp_type(audio_data):
        """The dtype calculate_true_peak returns (professional_meters.py:289-299): scipy's resample
        keeps float32 (and computes float16 in float32) and gives float64 for every other input, int
        frames and lists included; ``20 * np.log10`` keeps that type. Silence is the Python float
        -100.0 the reference returns (:295-296)."""
        dt = np.asarray(audio_data).dtype
        t = np.float32 if dt in (np.float32, np.float16) else np.float64
        return lambda v: -100.0 if v == -100.0 else t(v)

    def apply_k_weighting(self, audio_data: np.ndarray) -> np.ndarray:
        """professional_meters.py:129-153 (returned as float64 like scipy's filtfilt)."""
        return self._weighted(audio_data, "K")

    def create_k_weighting_filter(self):
        """professional_meters.py:48-72: second-order Butterworth high-passes at 38 Hz and at 1500 Hz
        (the reference's "simplified shelf": iirfilter(2, ..., btype='high', ftype='butter')) and the
        +4 dB shelf gain it computes but never applies (:59). The device builds the same coefficients
        for the K-weighting it runs (omega_k_weighting / omega_weighting)."""
        hp_b, hp_a = _butter2_highpass(38.0, self.sample_rate)
        sh_b, sh_a = _butter2_highpass(1500.0, self.sample_rate)
        return {"hp_b": hp_b, "hp_a": hp_a, "shelf_b": sh_b, "shelf_a": sh_a, "shelf_gain": 10 ** (4.0 / 20)}

    def create_a_weighting_filter(self):
        """professional_meters.py:74-107: the four cascaded Butterworth sections (the device builds the
        same coefficients in omega_weighting)."""
        fs, nyq = self.sample_rate, self.sample_rate / 2
        return {"hp1": _butter2_highpass(20.598997, fs), "hp2": _butter1(107.65265, fs, True),
                "lp1": _butter1(737.86223, fs, False), "lp2": _butter2_lowpass(min(12194.217 / nyq, 0.99) * nyq, fs),
                "gain": 1.0}

    def create_c_weighting_filter(self):
        """professional_meters.py:109-127."""
        fs, nyq = self.sample_rate, self.sample_rate / 2
        return {"hp": _butter2_highpass(20.598997, fs), "lp": _butter2_lowpass(min(12194.217 / nyq, 0.99) * nyq, fs),
                "gain": 1.0}

    def _weighted(self, audio_data, mode: str) -> np.ndarray:
        try:
            w, _ = self._eng.weighting(self._frame(audio_data), mode)
            return w[0].astype(np.float64)
        except Exception as e:
            logger.error("apply_%s_weighting: %s", mode.lower(), e)
            return np.zeros(len(audio_data), np.float64)

    def apply_a_weighting(self, audio_data: np.ndarray) -> np.ndarray:
        """professional_meters.py:155-192: RMS gate, four cascaded filtfilt sections, times 2.5."""
        return self._weighted(audio_data, "A")

    def apply_c_weighting(self, audio_data: np.ndarray) -> np.ndarray:
        """professional_meters.py:194-218: RMS gate, two cascaded filtfilt sections."""
        return self._weighted(audio_data, "C")

    def apply_weighting(self, audio_data: np.ndarray) -> np.ndarray:
        """professional_meters.py:220-229: K, A and C on the device; any other mode is Z (unweighted)."""
        if self.weighting_mode not in ("K", "A", "C"):
            return audio_data
        return self._weighted(audio_data, self.weighting_mode)

    def calculate_true_peak(self, audio_data: np.ndarray, oversampling: int = 4) -> float:
        """professional_meters.py:283-299 (the result follows the input dtype like scipy's resample:
        float32 for float32 frames, float64 for the app's float64 Hann frames, omega4_main.py:1082)."""
        if len(audio_data) == 0:
            return -100.0
        try:
            tp = self._eng.true_peak(self._frame(audio_data), oversampling)[0]
            self.current_true_peak = self._tp_type(audio_data)(tp)
        except Exception as e:
            logger.error("calculate_true_peak: %s", e)
        return self.current_true_peak

    def _meters(self, frames) -> np.ndarray:
        """The [F, 5] dict values of frames [F, M] of this stream in order, the device's state advanced by them:
        weighting + true peak + aggregates in one round trip. Raises what the library refuses."""
        mode = "Z" if self.weighting_mode not in ("K", "A", "C") else self.weighting_mode
        return self._eng.calculate_lufs(frames, mode)[2]

    def _take(self, m, audio_data) -> Dict[str, float]:
        """One row of _meters into the dict."""
        self.current_lufs["momentary"] = np.float64(m[0])
        self.current_lufs["short_term"] = np.float64(m[1])
        self.current_lufs["integrated"] = np.float64(m[2])
        self.current_lufs["range"] = np.float64(m[3])
        self.current_lufs["true_peak"] = self._tp_type(audio_data)(m[4])
        return self.current_lufs

    def calculate_lufs(self, audio_data: np.ndarray) -> Dict[str, float]:
        """professional_meters.py:231-281."""
        if len(audio_data) == 0:
            return self.current_lufs
        try:
            m = self._meters(self._frame(audio_data))[0]
        except Exception as e:
            logger.error("calculate_lufs: %s", e)
            return self.current_lufs
        return self._take(m, audio_data)

    def calculate_lufs_batch(self, frames: np.ndarray) -> np.ndarray:
        """Batched form: frames [F, M] of one stream in order -> [F, 5] dict values per call."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        mode = "Z" if self.weighting_mode not in ("K", "A", "C") else self.weighting_mode
        _, li = self._eng.weighting(frames, mode, weighted=False)
        tp = self._eng.true_peak(frames)
        return self._eng.meter_update(li, tp, frames.shape[0])

    def reset(self):
        self._eng.reset_meters()
        self.current_lufs.update({"momentary": -100.0, "short_term": -100.0, "integrated": -100.0, "range": 0.0,
                                  "true_peak": -100.0})


# omega_meterpanel_update's row columns (include/omega.h)
ROW_HOLD, ROW_COUNTER, ROW_ATTACK, ROW_PUNCH, ROW_COUNT, ROW_FLAGS, ROW_FILL, ROW_SUM = range(8)
ROW_COLS = 8
FLAG_ATTACK, FLAG_NONFINITE = 1, 2
MAX_FRAME = 16384


class ProfessionalMetersPanel:
    """ProfessionalMetersPanel (omega4/panels/professional_meters.py:302-397, :516-579) without the drawing.

        p = ProfessionalMetersPanel(48000)
        p.update(audio_windowed)                 # what the main loop feeds the panel
        p.get_results()                          # {'lufs': ..., 'transient': ...}
        rows, hist = p.update_batch(frames)      # [F, M] of the stream in order -> [F, 8] float64, [F, 60] int32
        p._panel_rows(frames, meters, state)     # omega_meterpanel_update itself, device tensors included

    update is one calculate_lufs on this panel's ``metering`` followed by one omega_meterpanel_update, which does on
    the device everything else the reference's update does: the three histories, the level histogram, the peak hold
    and the transient scan over the frame's samples, in the frame's dtype (float32 and float64 frames are kept;
    anything else is scanned as float64, which is exact for the integer types; include/omega.h has the definitions
    and the row layout). The panel's state is a blob this object carries from call to call; the histories, the hold
    and its counter read from it (omega_meterpanel_unpack). Frames of 1..16384 samples are built. Errors are logged
    and every value stays, as in ProfessionalMetering: the reference raises from scipy's filtfilt for a frame of 9
    samples or fewer, before it has changed anything. That holds for what is refused up front, a frame length the
    metering or the panel does not take; the metering's device state moves before the panel's call, so a failure of
    that call itself (an allocation, the device) leaves this object's values but not the metering's windows.
    Deviation: a frame that is neither float32 nor float64 (float16, integers) is scanned as float64, where the
    reference takes ``diff(|x|) > 0.1`` in the frame's own dtype; for integers the two agree. ``level_len`` /
    ``peak_len`` / ``range_len``, beyond the reference's signature, are the three deques' maxlen (600 / 300 / 300
    there, where a caller replaces the deques after construction); ``_n_bins`` / ``_hist_lo`` / ``_hist_hi`` are the
    tests' way to other edges."""

    def __init__(self, sample_rate: int = 48000, device: int = 0, level_len: int = 600, peak_len: int = 300,
                 range_len: int = 300, _n_bins: int = 60, _hist_lo: float = -60.0, _hist_hi: float = 0.0):
        self._host_init(sample_rate, level_len, peak_len, range_len, _n_bins, _hist_lo, _hist_hi)
        self.metering = ProfessionalMetering(sample_rate, device)
        self._eng = self.metering._eng

    def _host_init(self, sample_rate, level_len: int = 600, peak_len: int = 300, range_len: int = 300,
                   n_bins: int = 60, hist_lo: float = -60.0, hist_hi: float = 0.0) -> None:
        """The state that needs no device (:305-339)."""
        self.sample_rate = sample_rate
        self.transient_info = {'attack_time': 0.0, 'punch_factor': 0.0, 'transients_detected': 0}
        self._cfg = L.MeterPanelConfig()
        L.lib().omega_meterpanel_config_default(C.byref(self._cfg))
        self._cfg.sample_rate = float(sample_rate)
        self._cfg.level_len, self._cfg.peak_len, self._cfg.range_len = int(level_len), int(peak_len), int(range_len)
        self._cfg.n_bins, self._cfg.hist_lo, self._cfg.hist_hi = int(n_bins), float(hist_lo), float(hist_hi)
        n = L.lib().omega_meterpanel_state_size(C.byref(self._cfg))
        L.check_plain(min(n, 0), "omega_meterpanel_state_size: bad sample rate or history lengths")
        self._state_len = int(n)
        self.histogram_bins = np.empty(self._cfg.n_bins + 1, np.float64)
        L.check_plain(L.lib().omega_meterpanel_edges(C.byref(self._cfg), self.histogram_bins.ctypes.data),
                      "omega_meterpanel_edges")
        self.peak_hold_time = 1.0
        self.peak_hold_samples = int(self.peak_hold_time * 60)
        self.use_gated_measurement = True
        self.font_large = self.font_medium = self.font_small = self.font_meters = None
        self._state = None        # the blob (None: a new panel)
        self._reset_hold = False  # reset_peak_hold since the last update
        self._hist = None         # the last frame's histogram counts
        self._tp = float          # the type of the true peak the hold last saw
        self._configured = None

    # -- what reads from the blob --
    def _unpack(self):
        c = self._cfg
        lv, pk, rg = np.empty(c.level_len), np.empty(c.peak_len), np.empty(c.range_len)
        n = (C.c_int32 * 3)()
        hold, tr = np.empty(2), np.empty(3)
        a, i32 = C.addressof(n), C.sizeof(C.c_int32)
        L.check_plain(L.lib().omega_meterpanel_unpack(C.byref(c), self._state.ctypes.data, lv.ctypes.data, a,
                                                      pk.ctypes.data, a + i32, rg.ctypes.data, a + 2 * i32,
                                                      hold.ctypes.data, tr.ctypes.data), "omega_meterpanel_unpack")
        return lv[:n[0]], pk[:n[1]], rg[:n[2]], hold, tr

    def _history(self, k: int, maxlen: int) -> deque:
        return deque([] if self._state is None else list(self._unpack()[k]), maxlen=maxlen)

    @property
    def level_history(self) -> deque:
        return self._history(0, self._cfg.level_len)

    @property
    def true_peak_history(self) -> deque:
        return self._history(1, self._cfg.peak_len)

    @property
    def loudness_range_history(self) -> deque:
        return self._history(2, self._cfg.range_len)

    @property
    def peak_hold_value(self):
        if self._reset_hold or self._state is None:
            return -100.0
        v = self._unpack()[3][0]
        return -100.0 if v == -100.0 else self._tp(v)

    @property
    def peak_hold_counter(self) -> int:
        return 0 if self._reset_hold or self._state is None else int(self._unpack()[3][1])

    # -- the device part --
    def _configure(self, m: int) -> None:
        if not 1 <= m <= MAX_FRAME:
            raise L.UnsupportedError(L.EUNSUP, f"meterpanel: {m} samples per frame (1..{MAX_FRAME} are built)")
        if self._configured != m:
            cfg = L.MeterPanelConfig.from_buffer_copy(self._cfg)
            cfg.frame_len = int(m)
            # (a refused shape leaves the configured one as it was)
            self._eng._check(L.lib().omega_meterpanel_configure(self._eng._ctx, C.byref(cfg)))
            self._configured = m

    def _panel_rows(self, frames, meters, state=None, reset_hold: bool = False, hist: bool = True):
        """omega_meterpanel_update on frames [F, m] (float32 / float64; host numpy, or a device torch tensor whose
        rows may overlap) and their meters [F, 5] float64. state: what an earlier call returned, or None for a new
        panel. Returns (rows [F, 8] float64, hist [F, n_bins] int32 or None, the new state). Nothing of this object
        changes but the configured frame length."""
        dev = M._is_torch(frames)
        frames, frame_ptr, stride, f64 = M.rows(frames, dev, "frames must be [F, m]", audio=True)
        F, m = frames.shape
        self._configure(m)
        if dev:
            import torch
            meters = torch.as_tensor(meters, dtype=torch.float64, device=frames.device).contiguous()
            if tuple(meters.shape) != (F, L.N_METERS):
                raise ValueError("meters must be [F, 5]")
        else:
            meters = np.ascontiguousarray(meters, np.float64)
            if meters.shape != (F, L.N_METERS):
                raise ValueError("meters must be [F, 5]")
        state = M.state_blob(state, frames, self._state_len)
        rows = M.alloc(frames, (F, ROW_COLS), np.float64)
        counts = M.alloc(frames, (F, self._cfg.n_bins), np.int32) if hist else None
        new = M.alloc(frames, (self._state_len,), np.float64)
        M.call(self._eng, L.lib().omega_meterpanel_update, frames, frame_ptr, stride, f64, _ptr(meters), F,
               int(self.peak_hold_samples), int(bool(reset_hold)), _ptr(state), _ptr(rows), _ptr(counts), _ptr(new))
        return rows, counts, new

    def _run(self, frames: np.ndarray, what: str):
        """update / update_batch: frames [F, M] through the metering and the panel; None where it failed."""
        try:
            frames = np.asarray(frames)
            if frames.dtype not in (np.float32, np.float64):
                frames = frames.astype(np.float64)
            self._configure(frames.shape[1])  # (refused before the metering's state moves)
            meters = self.metering._meters(np.ascontiguousarray(frames, np.float32))
            rows, hist, new = self._panel_rows(frames, meters, self._state, self._reset_hold)
        except Exception as e:
            logger.error("%s: %s", what, e)
            return None
        self.lufs_info = self.metering._take(meters[-1], frames)
        self._tp = self.metering._tp_type(frames)
        self._state, self._reset_hold, self._hist = new, False, hist[-1].astype(np.int64)
        hit = np.flatnonzero(rows[:, ROW_FLAGS].astype(np.int64) & FLAG_ATTACK)
        if len(hit):  # (the three values keep the last attack's; without one in the call they stay)
            r = rows[-1]
            self.transient_info['attack_time'] = np.float64(r[ROW_ATTACK])
            self.transient_info['punch_factor'] = frames.dtype.type(r[ROW_PUNCH]) if r[ROW_PUNCH] != 0 else 0.0
            self.transient_info['transients_detected'] = int(r[ROW_COUNT])
        return rows, hist

    # -- the reference's surface --
    def set_fonts(self, fonts) -> None:
        """:341-346; nothing is drawn."""
        self.font_large = fonts.get('large')
        self.font_medium = fonts.get('medium')
        self.font_small = fonts.get('small')
        self.font_meters = fonts.get('meters', fonts.get('small'))

    def update(self, audio_data) -> None:
        """:348-397."""
        self._run(np.asarray(audio_data).reshape(1, -1), "update")

    def update_batch(self, frames):
        """frames [F, M] of the stream in order: (rows [F, 8], hist [F, n_bins]) as omega_meterpanel_update writes
        them, the panel's attributes left at the last frame; None where the call failed (logged)."""
        return self._run(frames, "update_batch")

    def get_results(self) -> Dict[str, Any]:
        """:542-547."""
        return {'lufs': self.lufs_info if hasattr(self, 'lufs_info') else None, 'transient': self.transient_info}

    def set_weighting(self, mode: str) -> None:
        if mode in ['K', 'A', 'C', 'Z']:
            self.metering.weighting_mode = mode

    def set_peak_hold_time(self, seconds: float) -> None:
        self.peak_hold_time = max(0.0, seconds)
        self.peak_hold_samples = int(self.peak_hold_time * 60)

    def toggle_gating(self) -> None:
        self.use_gated_measurement = not self.use_gated_measurement

    def reset_peak_hold(self) -> None:
        """:563-566 (applied on the device before the next frame)."""
        self._reset_hold = True

    def get_level_histogram(self) -> Tuple[np.ndarray, np.ndarray]:
        """:568-579 from the device's counts."""
        if self._hist is None:
            return self.histogram_bins[:-1], np.zeros(len(self.histogram_bins) - 1)
        hist = self._hist
        if hist.sum() > 0:
            hist = hist.astype(float) / hist.sum()
        return self.histogram_bins[:-1], hist

    def get_lufs_color(self, lufs_value: float) -> Tuple[int, int, int]:
        """:516-527."""
        if lufs_value > -9:
            return (255, 100, 100)
        elif lufs_value > -14:
            return (255, 200, 100)
        elif lufs_value > -23:
            return (100, 255, 100)
        elif lufs_value > -35:
            return (180, 180, 255)
        return (120, 120, 120)

    def get_peak_color(self, peak_db: float) -> Tuple[int, int, int]:
        """:529-540."""
        if peak_db > -0.1:
            return (255, 50, 50)
        elif peak_db > -3:
            return (255, 150, 50)
        elif peak_db > -6:
            return (100, 255, 100)
        elif peak_db > -20:
            return (180, 200, 220)
        return (120, 120, 120)

    def reset(self) -> None:
        """A new panel: the metering's device state, this panel's blob and the transient values."""
        self.metering.reset()
        self._state, self._reset_hold, self._hist, self._tp = None, False, None, float
        self.transient_info.update({'attack_time': 0.0, 'punch_factor': 0.0, 'transients_detected': 0})
        if hasattr(self, 'lufs_info'):
            del self.lufs_info
