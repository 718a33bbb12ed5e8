"""A numpy restatement of omega_rhythm_features' columns (include/omega.h) from the expressions of
omega4/panels/beat_detection.py and omega4/panels/frequency_band_tracker.py, for consecutive frames of one stream
chained through the state blob the library uses. TEST INFRASTRUCTURE ONLY. Every sum the device forms in float64
is taken with math.fsum here (the reference sums the float32 spectrum in float32; tests/test_rhythm.py derives what
that costs). The flux difference is numpy's own float32 subtraction, as in the reference.
"""
import math

import numpy as np

COLUMNS = ("flags", "sumsq", "spec_sum", "flux", "kick", "band0", "band1", "band2", "band3", "band4", "band5",
           "band6", "spec_fsum", "spread_sum")
FLAG_NONFINITE, FLAG_GATED, FLAG_NO_FLUX = 1, 2, 4
EDGE_HZ = (20, 50, 60, 120, 250, 500, 2000, 4000, 8000, 20000)
UPPER_ONLY = (3, 9)  # 120 and 20000 Hz are never a band's lower edge
KICK = (1, 3)
BANDS = ((0, 2), (2, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9))
GATE = 0.001


def fsum(v):
    return math.fsum(np.asarray(v, np.float64).ravel().tolist())


def state_len(K):
    return 2 + K


def edges(freqs):
    """np.argmax(freqs >= f) per edge, as beat_detection.py:85-89 and frequency_band_tracker.py:118-122 find
    them; where that gives 0 for an edge that is only ever an upper one, len(freqs)."""
    freqs = np.asarray(freqs)
    e = [int(np.argmax(freqs >= f)) for f in EDGE_HZ]
    for i in UPPER_ONLY:
        if e[i] == 0:
            e[i] = len(freqs)
    return tuple(e)


def band_range(e, lo, hi, K):
    """The reference's slice for a band: the upper index 0 means 'beyond the spectrum' and reads as K."""
    return e[lo], (K if e[hi] == 0 else e[hi])


def row(spec, x, freqs, state=None):
    """One frame's columns and the stream's new state. spec: K float32 values; x: m samples or None (the
    tracker's call); freqs: K float64; state: the blob an earlier frame returned, or None."""
    spec = np.asarray(spec, np.float32)
    freqs = np.asarray(freqs, np.float64)
    K = len(spec)
    state = np.zeros(state_len(K)) if state is None else np.asarray(state, np.float64)
    has_state = state[0] != 0 and state[1] == K
    if not has_state:  # what the library writes where no live frame has come yet
        state = np.zeros(state_len(K))
        state[1] = K
    r = np.zeros(len(COLUMNS))
    xd = None if x is None else np.asarray(x, np.float64)
    if not (np.all(np.isfinite(spec)) and (xd is None or np.all(np.isfinite(xd)))):
        r[0] = FLAG_NONFINITE
        return r, state.copy()
    flags = 0
    if xd is not None:
        r[1] = fsum(xd * xd)
        if math.sqrt(r[1] / len(xd)) < GATE:
            flags |= FLAG_GATED
    s64 = spec.astype(np.float64)
    r[2] = fsum(s64)
    if has_state:
        prev = state[2:].astype(np.float32)
        r[3] = fsum(np.maximum(0, spec - prev))  # :71 (float32 differences)
    else:
        flags |= FLAG_NO_FLUX
    e = edges(freqs)
    lo, hi = band_range(e, *KICK, K)
    r[4] = fsum(s64[lo:hi])
    for b, (i, j) in enumerate(BANDS):
        lo, hi = band_range(e, i, j, K)
        r[5 + b] = fsum(s64[lo:hi])
    r[12] = fsum(freqs * s64)
    total = float(np.float32(r[2]))
    if total > 0:
        c = r[12] / total
        if c > 0:
            r[13] = fsum((freqs - c) ** 2 * s64)
    r[0] = flags
    if flags & FLAG_GATED:
        return r, state.copy()
    new = np.zeros(state_len(K))
    new[0], new[1] = 1, K
    new[2:] = s64
    return r, new


def rows(spectra, frames, freqs, state=None):
    out = []
    for i, s in enumerate(spectra):
        r, state = row(s, None if frames is None else frames[i], freqs, state)
        out.append(r)
    return np.array(out).reshape(-1, len(COLUMNS)), state
