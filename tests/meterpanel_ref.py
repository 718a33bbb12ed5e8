"""numpy restatement of what ProfessionalMetersPanel.update (omega4/panels/professional_meters.py:348-397, :568-579)
does with a frame and with the dict calculate_lufs returned for it, in the row and blob layout of
omega_meterpanel_update (include/omega.h). tests/golden/gen_meterpanel.py asserts it against the reference object after
every frame; the tests use it to build blobs and expected rows."""
from collections import deque

import numpy as np

HEAD = 16
ROW_COLS = 8
FLAG_ATTACK, FLAG_NONFINITE = 1, 2
KEYS = ("momentary", "short_term", "integrated", "range", "true_peak")


def frame_record(x):
    """(attack count, first attack index or -1, punch factor in x's dtype or 0.0, a non-finite sample) of one frame,
    in the reference's expressions (:376-397)."""
    x = np.asarray(x)
    bad = not np.all(np.isfinite(x))
    if len(x) <= 1:
        return 0, -1, 0.0, bad
    idx = np.where(np.diff(np.abs(x)) > 0.1)[0]
    if len(idx) == 0:
        return 0, -1, 0.0, bad
    with np.errstate(all="ignore"):
        rms = np.sqrt(np.mean(x ** 2))
        peak = np.max(np.abs(x))
        punch = peak / rms if rms > 0 else 0.0
    return len(idx), int(idx[0]), punch, bad


def bin_counts(values, edges):
    """np.histogram(values, edges)[0] by the definition: edges[b] <= v < edges[b + 1], the last bin closed."""
    n = len(edges) - 1
    out = np.zeros(n, np.int64)
    for v in values:
        if not (v >= edges[0]) or v > edges[-1]:
            continue
        out[n - 1 if v == edges[-1] else int(np.searchsorted(edges, v, side="right")) - 1] += 1
    return out


class Panel:
    def __init__(self, sample_rate=48000, level_len=600, peak_len=300, range_len=300, n_bins=60, lo=-60.0, hi=0.0):
        self.sample_rate = sample_rate
        self.level, self.peaks, self.ranges = deque(maxlen=level_len), deque(maxlen=peak_len), deque(maxlen=range_len)
        self.pushed = 0
        self.edges = np.linspace(lo, hi, n_bins + 1)
        self.hold, self.counter = -100.0, 0
        self.attack, self.punch, self.count = 0.0, 0.0, 0

    def reset_peak_hold(self):
        self.hold, self.counter = -100.0, 0

    def step(self, x, meters, hold_samples):
        """One update; returns (row [8], the histogram's counts)."""
        self.level.append(meters[0])
        self.ranges.append(meters[3])
        self.peaks.append(meters[4])
        self.pushed += 1
        cur = meters[4]
        if cur > self.hold:
            self.hold, self.counter = cur, int(hold_samples)
        else:
            self.counter -= 1
            if self.counter <= 0:
                self.hold = cur
        n, first, punch, bad = frame_record(x)
        if n:
            self.attack = (np.int64(first) / self.sample_rate) * 1000
            self.punch, self.count = punch, n
        hist = bin_counts(self.level, self.edges)
        flags = (FLAG_ATTACK if n else 0) | (FLAG_NONFINITE if bad else 0)
        row = np.array([self.hold, self.counter, self.attack, self.punch, self.count, flags, len(self.level),
                        hist.sum()], np.float64)
        return row, hist

    def blob(self):
        """The state as omega_meterpanel_update writes it: a ring fills from slot 0 and then wraps."""
        lens = [d.maxlen for d in (self.level, self.peaks, self.ranges)]
        out = np.zeros(HEAD + sum(lens))
        out[:5] = [self.hold, self.counter, self.attack, self.punch, self.count]
        off = HEAD
        for k, d in enumerate((self.level, self.peaks, self.ranges)):
            L, pos = d.maxlen, self.pushed % d.maxlen
            out[5 + 2 * k], out[6 + 2 * k] = len(d), pos
            for i, v in enumerate(d):  # oldest first: slot pos when full, slot 0 before
                out[off + ((pos + i) % L if len(d) == L else i)] = v
            off += L
        return out


def run(frames, meters, hold_samples, resets=None, **kw):
    """rows [F, 8], hists [F, n_bins] int32 and the final Panel of a stream."""
    p = Panel(**kw)
    rows, hists = [], []
    for i, x in enumerate(frames):
        if resets is not None and resets[i]:
            p.reset_peak_hold()
        r, h = p.step(x, meters[i], hold_samples[i])
        rows.append(r)
        hists.append(h)
    return np.array(rows), np.array(hists, np.int32), p
