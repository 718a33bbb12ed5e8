"""SpectrogramWaterfall (omega4/panels/spectrogram_waterfall.py:56-121, :142-205, :295-305) restated in numpy, in the
reference's types under numpy 2.x: float32 spectra give float32 dB rows, maxima, percentiles and rows, float64
spectra float64, Python scalars are weak. One difference on purpose: log10 is taken in float64 of the exactly widened
value and rounded once (the device's rule); the reference's float32 chain goes through the C library's log10f, which
is not correctly rounded (tests/test_waterfall.py states the bar this costs).

This project's rule for a frame with a non-finite bin: flag bit 0, a zero row, and the state goes on as if the frame
had not come.
"""
import numpy as np

SCHEMES = ("spectrum", "hot", "cool", "viridis")  # the library's scheme ids; any other id is the grey fallback
GREY = 4
HISTORY = 20
COLS = ("flags", "db_max", "db_min", "peak", "floor", "argmax", "argmax_value")
F32_BAR = 8 * 2.0 ** -24  # rows, absolute (tests/test_waterfall.py derives it)


def widen(s32):
    """The float64 sequence that goes with a recorded float32 one: every value moved off the float32 grid by one
    IEEE product (zeros stay zeros), so that the golden file stores the float32 spectra only."""
    return s32.astype(np.float64) * (1.0 + 2.0 ** -30)


def mapping(sample_rate, fft_size, min_freq, max_freq):
    """_setup_frequency_mapping (:56-69) -> (min_idx, max_idx)."""
    bins = np.linspace(0, sample_rate / 2, fft_size // 2 + 1)
    lo = int(np.argmax(bins >= min_freq))
    hi = int(np.argmax(bins >= max_freq))
    if hi == 0:
        hi = len(bins) - 1
    return lo, hi


def percentile_pair(maxima, minima):
    """:95-100 on the recorded history: lists of numpy scalars of one type, the newest last."""
    return np.percentile(list(maxima)[-HISTORY:], 95), np.percentile(list(minima)[-HISTORY:], 5)


def percentile_stage(maxima, minima, dtype):
    """Frame i's (peak, floor) from the maxima and minima of frames 0..i, as the reference's sliding window."""
    mx = [dtype(v) for v in maxima]
    mn = [dtype(v) for v in minima]
    out = [percentile_pair(mx[:i + 1], mn[:i + 1]) for i in range(len(mx))]
    return np.array([o[0] for o in out], dtype), np.array([o[1] for o in out], dtype)


def db_row(x):
    """:85 with log10 in float64."""
    m = np.maximum(x, 1e-10)
    return 20 * np.log10(m.astype(np.float64)).astype(x.dtype)


class Waterfall:
    """The update step (:71-121) on one slice; `history` holds every (max, min) so far."""

    def __init__(self):
        self.auto_gain = True
        self.gain_adjustment = 0.0
        self.current_peak = 0.0
        self.current_floor = -80.0
        self.history = []

    def update(self, x, lo, hi):
        """One frame's spectrum -> (flags, row, db_max, db_min); x keeps its type (float32 or float64)."""
        sl = x[lo:hi]
        if not np.all(np.isfinite(x)):
            return 1, np.zeros_like(sl), x.dtype.type(0), x.dtype.type(0)
        db = db_row(sl)
        mx, mn = np.max(db), np.min(db)
        self.history.append((mx, mn))
        if self.auto_gain:
            self.current_peak, self.current_floor = percentile_pair([h[0] for h in self.history],
                                                                    [h[1] for h in self.history])
        adjusted = db + self.gain_adjustment
        span = self.current_peak - self.current_floor
        row = (adjusted - self.current_floor) / span if span > 0 else np.zeros_like(adjusted)
        return 0, np.clip(row, 0.0, 1.0), mx, mn


def run(spectra, lo, hi, auto_gain=True, gain=0.0, wf=None):
    """Frames [F, n] through one Waterfall -> (stats [F, 7] float64, rows [F, cells])."""
    wf = wf or Waterfall()
    wf.auto_gain, wf.gain_adjustment = auto_gain, gain
    stats, rows = [], []
    for x in spectra:
        flags, row, mx, mn = wf.update(x, lo, hi)
        if flags:
            stats.append([1.0, 0, 0, 0, 0, 0, 0])
        else:
            k = int(np.argmax(x))
            stats.append([0.0, float(mx), float(mn), float(wf.current_peak), float(wf.current_floor), k, float(x[k])])
        rows.append(row)
    return np.array(stats, np.float64).reshape(len(rows), len(COLS)), np.array(rows, spectra.dtype)


def colors(x, scheme):
    """_spectrum_to_color (:142-205) over an array of float32 or float64 intensities -> uint8 [..., 3]. Every
    expression is the reference's, evaluated on the whole array in its type (Python literals are weak); int() is
    astype's truncation."""
    x = np.asarray(x)
    dt = x.dtype.type
    with np.errstate(invalid="ignore"):
        x = np.where(x < 1.0, x, dt(1.0))  # max(0.0, min(1.0, intensity))
        x = np.where(x > 0.0, x, dt(0.0))
    z, full = np.zeros(x.shape, np.int64), np.full(x.shape, 255, np.int64)
    tr = lambda v: v.astype(np.int64)  # noqa: E731
    if scheme == 0:
        c = [x < 0.25, x < 0.5, x < 0.75]
        r = np.select(c, [z, z, tr(255 * ((x - 0.5) / 0.25))], full)
        g = np.select(c, [tr(255 * (x / 0.25)), full, full], tr(255 * (1 - (x - 0.75) / 0.25)))
        b = np.select(c, [full, tr(255 * (1 - (x - 0.25) / 0.25)), z], z)
    elif scheme == 1:
        c = [x < 0.33, x < 0.66]
        r = np.select(c, [tr(255 * (x / 0.33)), full], full)
        g = np.select(c, [z, tr(255 * ((x - 0.33) / 0.33))], full)
        b = np.select(c, [z, z], tr(255 * ((x - 0.66) / 0.34)))
    elif scheme == 2:
        r, g, b = tr(255 * x), tr(255 * (1 - x)), full
    elif scheme == 3:
        h, s, v = 0.8 - 0.8 * x, 0.9, 0.2 + 0.8 * x
        h6 = h * 6.0  # colorsys.hsv_to_rgb
        i = tr(h6)
        f = h6 - i.astype(x.dtype)
        p = v * (1.0 - s)
        q = v * (1.0 - s * f)
        t = v * (1.0 - s * (1.0 - f))
        i = i % 6
        pick = lambda *a: np.select([i == k for k in range(5)], a[:5], a[5])  # noqa: E731
        r, g, b = (tr(pick(*a) * 255) for a in ((v, q, p, p, t, v), (t, v, v, q, p, p), (p, p, t, v, v, q)))
    else:
        r = g = b = tr(255 * x)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)
