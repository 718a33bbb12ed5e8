"""The stereo phase correlation analysis restated in numpy from its formulas (TEST INFRASTRUCTURE ONLY): what
omega4/panels/phase_correlation.py:124-220 computes from a left and a right channel, as the row and the
points of include/omega.h's omega_phase_correlation. tests/test_phase.py pins it to tests/golden/phase.npz
(the reference's own outputs) bit for bit on the recorded numpy; everything is float64, the reference's
precision for float64 arrays.
"""
import math

import numpy as np

COLUMNS = ("correlation", "stereo_width", "balance", "rms_left", "rms_right", "flags", "band_mask") + tuple(
    f"band_{b}" for b in range(10))
N_BANDS, N_COLS, N_POINTS = 10, 17, 128
FLAG_NONFINITE, FLAG_NO_ENERGY, FLAG_FLAT = 1, 2, 4
MIN_FRAME, MAX_FRAME = 64, 8192


def band_edges(fs):
    """The 11 logarithmic band edges from 20 Hz to min(20 kHz, Nyquist)."""
    return np.logspace(np.log10(20), np.log10(min(20000, fs / 2)), N_BANDS + 1)


def band_ranges(fs, m, edges=None):
    """[10, 2] first and one-past-last rfft bin of every band: lo <= f_k < hi over np.fft.rfftfreq."""
    edges = band_edges(fs) if edges is None else edges
    freqs = np.fft.rfftfreq(m, 1 / fs)
    out = np.zeros((N_BANDS, 2), np.int32)
    for b in range(N_BANDS):
        idx = np.flatnonzero((freqs >= edges[b]) & (freqs < edges[b + 1]))
        if len(idx):
            out[b] = idx[0], idx[-1] + 1
    return out


def n_points(m):
    step = max(1, m // 100)
    return -(-m // step)


def pearson(a, b):
    """(clipped correlation of the mean-centred vectors, whether the 0.0 fallback was taken)."""
    ac, bc = a - np.mean(a), b - np.mean(b)
    sa, sb = np.std(ac), np.std(bc)
    if sa > 0 and sb > 0:
        return float(np.clip(np.mean(ac * bc) / (sa * sb), -1.0, 1.0)), False
    return 0.0, True


def points(left, right):
    """[128, 2] goniometer points of every step-th sample, zero past their number."""
    m = len(left)
    step = max(1, m // 100)
    l, r = left[::step], right[::step]
    mid, side = (l + r) / 2, (l - r) / 2
    out = np.zeros((N_POINTS, 2))
    out[:len(l), 0] = (mid - side) / math.sqrt(2) * 0.5
    out[:len(l), 1] = (mid + side) / math.sqrt(2) * 0.5
    return out


def features(left, right, fs, edges=None):
    """(row [17], points [128, 2]) of one stereo frame."""
    left, right = np.asarray(left, np.float64), np.asarray(right, np.float64)
    m = len(left)
    row = np.zeros(N_COLS)
    if not (np.isfinite(left).all() and np.isfinite(right).all()):
        row[5] = FLAG_NONFINITE
        return row, np.zeros((N_POINTS, 2))
    corr, flat = pearson(left, right)
    rl, rr = np.sqrt(np.mean(left ** 2)), np.sqrt(np.mean(right ** 2))
    total = rl + rr
    row[0], row[1] = corr, 1.0 - abs(corr)
    row[2] = (rr - rl) / total if total > 0 else 0.0
    row[3], row[4] = rl, rr
    row[5] = (0 if total > 0 else FLAG_NO_ENERGY) + (FLAG_FLAT if flat else 0)
    w = np.hanning(m)
    ml, mr = np.abs(np.fft.rfft(left * w)), np.abs(np.fft.rfft(right * w))
    mask = 0
    for b, (lo, hi) in enumerate(band_ranges(fs, m, edges)):
        if hi > lo:
            mask |= 1 << b
            row[7 + b] = pearson(ml[lo:hi], mr[lo:hi])[0]
    row[6] = mask
    return row, points(left, right)
