"""A numpy / scipy restatement of omega_tdetect_features' columns (include/omega.h) from the expressions of
omega4/panels/transient_detection.py, for consecutive frames of one stream chained through the state blob the
library uses. TEST INFRASTRUCTURE ONLY. Every sum the device forms in float64 is taken with math.fsum here (the
reference sums the float32 spectrum in float32; tests/test_transient_detection.py derives what that costs), and
the exact columns are decided in exact arithmetic: the golden generator asserts the margins that make them so.
"""
import math

import numpy as np
from scipy import signal

COLUMNS = ("flags", "envelope", "peak", "energy", "flux_sum", "flux", "novelty", "mag_sum", "hf_energy",
           "sign_diff", "peak_idx", "start_idx", "end_idx", "spec_sum", "spec_fsum", "rolloff_idx",
           "band0", "band1", "band2", "band3", "guards")
FLAG_NONFINITE, FLAG_NO_HF, FLAG_NO_NOVELTY_SHAPE, FLAG_NO_FLUX, FLAG_NO_NOVELTY = 1, 2, 4, 8, 16
FLUX_BINS, PHASE_BINS = 128, 513
STATE_LEN = 4 + FLUX_BINS + 2 * PHASE_BINS
EXACT = (0, 2, 9, 10, 11, 12, 15, 20)


def fsum(v):
    return math.fsum(np.asarray(v, np.float64).ravel().tolist())


def freqs_of(K, fs):
    return np.fft.rfftfreq((K - 1) * 2, 1 / fs)  # :222-223


def band_indices(K, fs):
    f = freqs_of(K, fs)
    return tuple(int(np.searchsorted(f, v)) for v in (0, 100, 250, 2000, fs / 2))  # :248-252


def flux_spectrum(x):
    """:152-166."""
    window = np.hanning(512)
    if len(x) >= 512:
        windowed = x[:512] * window
    else:
        padded = np.zeros(512)
        padded[:len(x)] = x
        windowed = padded * window
    return np.abs(np.fft.rfft(windowed))[:128]


def phase_spectrum(x):
    """:319-332 -> (phase, magnitude)."""
    pre = np.append(x[0], x[1:] - 0.97 * x[:-1])
    cur = np.fft.rfft(pre[-1024:] * np.hanning(1024))
    return np.angle(cur), np.abs(cur)


def hf_signal(x, fs):
    """:193-198."""
    b, a = signal.butter(4, 5000 / (fs / 2), btype='high')
    return signal.filtfilt(b, a, x)


def has_hf(m, fs):
    return m > 256 and 5000 / (fs / 2) < 1.0


def row(spec, x, fs, state=None):
    """One frame's columns and the stream's new state. spec: K float32 magnitudes; x: m float64 samples; state:
    the blob an earlier frame returned, or None."""
    spec = np.asarray(spec, np.float32)
    x = np.asarray(x, np.float64)
    K, m = len(spec), len(x)
    state = np.zeros(STATE_LEN) if state is None else np.asarray(state, np.float64)
    r = np.zeros(len(COLUMNS))
    if not (np.all(np.isfinite(spec)) and np.all(np.isfinite(x))):
        r[0] = FLAG_NONFINITE
        return r, state.copy()
    hf, nov = has_hf(m, fs), m >= 1024
    flags = (0 if hf else FLAG_NO_HF) | (0 if nov else FLAG_NO_NOVELTY_SHAPE)
    new = np.zeros(STATE_LEN)
    r[1] = np.mean(signal.savgol_filter(np.abs(signal.hilbert(x)), 11, 3))  # :123-131
    ax = np.abs(x)
    r[2] = np.max(ax)
    r[3] = fsum(x * x)
    S = flux_spectrum(x)
    r[4] = fsum(S)
    if state[0]:
        r[5] = fsum(np.maximum(0, S - state[4:4 + FLUX_BINS]))  # :173
    else:
        flags |= FLAG_NO_FLUX
    new[0] = 1
    new[4:4 + FLUX_BINS] = S
    if nov:
        ph, mag = phase_spectrum(x)
        r[7] = fsum(mag)
        o = 4 + FLUX_BINS
        if state[1]:
            p1, p2 = state[o:o + PHASE_BINS], state[o + PHASE_BINS:]
            dev = np.minimum(np.abs(ph - (2 * p1 - p2)), np.pi)  # :343-345
            r[6] = fsum(mag * dev)
            new[o + PHASE_BINS:] = p1
        else:
            flags |= FLAG_NO_NOVELTY
            new[o + PHASE_BINS:] = ph  # :364
        new[1] = 1
        new[o:o + PHASE_BINS] = ph
    else:
        flags |= FLAG_NO_NOVELTY
    if hf:
        y = hf_signal(x, fs)
        r[8] = fsum(y * y)
    r[9] = np.sum(np.abs(np.diff(np.sign(x))))  # :237
    pk = int(np.argmax(ax))                      # :285-313
    r[10] = pk
    below = np.nonzero(ax < 0.1 * ax[pk])[0]
    r[11] = max([i for i in below if i < pk], default=0)
    r[12] = min([i for i in below if i > pk], default=m - 1)
    s64 = spec.astype(np.float64)
    f = freqs_of(K, fs)
    total = fsum(s64)
    r[13] = total
    r[14] = fsum(f * s64)
    if total > 0:
        cum = np.array([fsum(s64[:i + 1]) for i in range(K)]) if K <= 64 else np.cumsum(s64)
        r[15] = min(int(np.searchsorted(cum, 0.85 * total)), K - 1)  # :240-243
    idx = band_indices(K, fs)
    guards = 0
    for b in range(4):
        if idx[b] < K and idx[b + 1] < K:  # :254
            guards |= 1 << b
            r[16 + b] = fsum(s64[idx[b]:idx[b + 1]])
    r[20] = guards
    r[0] = flags
    return r, new


def rows(spectra, frames, fs, state=None):
    out = []
    for s, x in zip(spectra, frames):
        r, state = row(s, x, fs, state)
        out.append(r)
    return np.array(out), state
