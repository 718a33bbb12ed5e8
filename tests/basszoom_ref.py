"""A numpy restatement of omega_basszoom_mapping and omega_basszoom_features (include/omega.h) from the behaviour of
omega4/panels/bass_zoom.py: the bar mapping of a sample rate, one frame's row, and the float32 smoothing and peak
hold with an explicit clock. TEST INFRASTRUCTURE ONLY. The arithmetic types are numpy 2.x's (NEP 50): a float32
value times a Python float is a float32 product; a float32 plus a float64 is a float64, rounded on store.
"""
import numpy as np

N_FFT = 8192
ROW_HEAD = 3  # flags, bass_max, scale_factor
FLAG_NONFINITE = 1
MAX_BARS = 64
STATE_LEN = 3 * MAX_BARS
HOLD_SECONDS = 3.0


class Mapping:
    """The bins of the 8192-point spectrum within 20..200 Hz, cut into bars of max(1, count // 31) bins."""

    def __init__(self, fs):
        freqs = np.fft.rfftfreq(N_FFT, 1 / fs)
        valid = np.nonzero((freqs >= 20) & (freqs <= 200))[0]
        self.fs = fs
        self.n_valid = len(valid)
        self.first_bin = int(valid[0]) if len(valid) else 0
        self.bins_per_bar = max(1, len(valid) // 31)
        self.groups = [[int(k) for k in valid[i:i + self.bins_per_bar]]
                       for i in range(0, len(valid), self.bins_per_bar)]
        self.freq_ranges = []
        for g in self.groups:
            lo, hi = freqs[g[0]], freqs[g[-1]]
            if self.freq_ranges:
                lo = max(lo, self.freq_ranges[-1][1])
            self.freq_ranges.append((lo, hi))
        self.n_bars = len(self.groups)
        centre = np.array([(lo + hi) / 2 for lo, hi in self.freq_ranges])
        self.comp = np.select([centre < 60, centre < 100, centre < 150], [0.3, 0.6, 1.0], 0.8) if self.n_bars else centre


def magnitudes(x):
    """abs(rfft) of the first min(len, 8192) samples under a Hann window of that length, zero-padded to 8192."""
    n = min(len(x), N_FFT)
    buf = np.zeros(N_FFT)
    buf[:n] = np.asarray(x[:n], np.float64) * np.hanning(n)
    return np.abs(np.fft.rfft(buf))


def frame_row(x, mp):
    """One frame's row: flags, bass_max, scale_factor, then the compressed value of each bar."""
    row = np.zeros(ROW_HEAD + mp.n_bars)
    x = np.asarray(x, np.float64)
    if not np.all(np.isfinite(x)):
        row[0] = FLAG_NONFINITE
        return row
    mag = magnitudes(x)
    raw = np.array([np.mean(mag[g]) for g in mp.groups]) * mp.comp
    top = max(0.0, float(np.max(raw)))
    scale = 1.0
    if top > 0:
        scale = 0.85 / top
        scale *= np.log10(max(1.0, top * 10)) / 2.0
    v = raw * scale
    row[1], row[2] = top, scale
    row[ROW_HEAD:] = np.where(v > 0.7, 0.7 + (v - 0.7) * 0.3, v)
    return row


def new_state():
    return np.zeros(STATE_LEN)


def step(state, row, now, n_bars):
    """The state after one row at time ``now``: (bars float32, peaks float32, timestamps float64, new blob). A
    flagged row leaves the state as it is."""
    state = np.asarray(state, np.float64)
    bars = state[:n_bars].astype(np.float32)
    peaks = state[MAX_BARS:MAX_BARS + n_bars].astype(np.float32)
    stamps = state[2 * MAX_BARS:2 * MAX_BARS + n_bars].copy()
    if not int(row[0]) & FLAG_NONFINITE:
        c = np.asarray(row[ROW_HEAD:], np.float64)
        rising = c > bars.astype(np.float64)
        keep = np.where(rising, np.float32(0.1), np.float32(0.6))      # float32 factors
        take = np.where(rising, 0.9, 0.4)                               # float64 factors
        mixed = (bars * keep).astype(np.float64) + c * take             # float32 product, float64 product and sum
        bars = np.clip(mixed.astype(np.float32), np.float32(0), np.float32(1))
        higher = bars > peaks
        expired = ~higher & (now - stamps > HOLD_SECONDS)
        peaks = np.where(higher, bars, np.where(expired, peaks * np.float32(0.95), peaks)).astype(np.float32)
        stamps = np.where(higher, now, stamps)
    new = state.copy()
    new[:n_bars] = bars
    new[MAX_BARS:MAX_BARS + n_bars] = peaks
    new[2 * MAX_BARS:2 * MAX_BARS + n_bars] = stamps
    return bars, peaks, stamps, new


def run(frames, times, mp, state=None):
    """A stream: (rows, bars, peaks, peak_times, state) as omega_basszoom_features returns them."""
    state = new_state() if state is None else state
    rows, bars, peaks, stamps = [], [], [], []
    for x, t in zip(frames, times):
        r = frame_row(x, mp)
        b, p, s, state = step(state, r, t, mp.n_bars)
        rows.append(r)
        bars.append(b)
        peaks.append(p)
        stamps.append(s)
    return np.array(rows), np.array(bars), np.array(peaks), np.array(stamps), state
