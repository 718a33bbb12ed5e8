"""Float64 restatement of the 4x true peak (professional_meters.py:283-299, scipy.signal.resample) and
the designed signals of tests/test_true_peak_phases.py. TEST INFRASTRUCTURE ONLY: the product does not
import it.

``phase_peaks(x)`` returns max |y[p::4]| for p = 0..3 of y = resample(x, 4N) evaluated in float64: phase 0
is the samples, phases 1..3 are the interpolated ones. The expected device values follow the tp_phases
masks of omega_true_peak_os: 1x = phase 0, 2x = phases 0 and 2, 4x = all four. ``nyq_scale`` replaces the
0.5 that resample puts on an even length's Nyquist bin, in the interpolated phases only; it exists to
prove on the CPU that a signal is sensitive to that weight and is never anything but 0.5 in a comparison
against the device.

Every builder returns float64; the tests cast to float32 and evaluate the reference on the cast frame.
"""
from __future__ import annotations

import functools

import numpy as np

SILENCE = 1e-10  # peak below which calculate_true_peak returns -100.0 (:295-296)


def resample4(x, nyq_scale=0.5):
    """rfft, copy bins 0..N//2, halve (nyq_scale) an even length's Nyquist bin, irfft(4N), scale 4."""
    x = np.asarray(x, np.float64)
    n = len(x)
    X = np.fft.rfft(x)
    Y = np.zeros(2 * n + 1, np.complex128)
    Y[: n // 2 + 1] = X[: n // 2 + 1]
    if n % 2 == 0:
        Y[n // 2] *= nyq_scale
    return np.fft.irfft(Y, 4 * n) * 4.0


def phase_peaks(x, nyq_scale=0.5):
    """[max |y[p::4]| for p in 0..3], float64."""
    y = resample4(x)
    if nyq_scale != 0.5:
        ys = resample4(x, nyq_scale)
        ys[0::4] = y[0::4]  # the samples themselves carry no interpolation weight
        y = ys
    return np.array([np.max(np.abs(y[p::4])) for p in range(4)])


def peak_of(phases, oversampling):
    """The peak the given oversampling factor sees: phase 0 / phases 0, 2 / all four."""
    sel = {1: [0], 2: [0, 2], 4: [0, 1, 2, 3]}[oversampling]
    return float(np.max(np.asarray(phases)[sel]))


def db(peak):
    """20 log10(peak), -100.0 below the silence threshold (float64)."""
    return -100.0 if peak < SILENCE else 20.0 * np.log10(peak)


def expected_db(x, oversampling, nyq_scale=0.5):
    return db(peak_of(phase_peaks(x, nyq_scale), oversampling))


# ---- signals (float64) ----

def tone(n, p):
    """0.5 cos(2 pi (N/4) (t - p/4) / N): its maxima fall on phase p (N divisible by 4)."""
    assert n % 4 == 0
    t = np.arange(n, dtype=np.float64)
    return 0.5 * np.cos(2 * np.pi * (n // 4) * (t - p / 4.0) / n)


def pulse_unscaled(n, c):
    """Band-limited pulse centred at the fractional position c: X[k] = exp(-2 pi i k c / N) for
    k = 0..(N-1)//2, no Nyquist term for an even N."""
    k = np.arange(n // 2 + 1, dtype=np.float64)
    X = np.exp(-2j * np.pi * k * c / n)
    if n % 2 == 0:
        X[n // 2] = 0.0
    return np.fft.irfft(X, n)


def pulse(n, c, peak=0.5):
    """The pulse scaled so that its 4x peak is `peak`."""
    x = pulse_unscaled(n, c)
    return x * (peak / phase_peaks(x).max())


def nyquist(n, a=0.5):
    assert n % 2 == 0
    return a * np.cos(np.pi * np.arange(n, dtype=np.float64))


def nyquist_mix_pulse(n, p):
    """Pulse on phase p (1 or 3) plus a Nyquist tone that adds to it at its centre: the interpolated
    winner carries the Nyquist bin with weight cos(pi/4)."""
    assert n % 2 == 0 and p in (1, 3)
    n0 = n // 3
    x = pulse(n, n0 + p / 4.0, 0.42)
    sign = np.cos(np.pi * n0) * np.cos(np.pi * p / 4.0)  # sign of cos(pi t) at t = n0 + p/4
    return x + nyquist(n, 0.05 * np.sign(sign))


def nyquist_mix_tone(n, p):
    """Tone on phase p (1 or 3) plus a Nyquist tone adding to its maximum at t = p/4 (N divisible by 4)."""
    assert p in (1, 3)
    return 0.9 * tone(n, p) + nyquist(n, 0.05 * np.sign(np.cos(np.pi * p / 4.0)))


def dc(n):
    return np.full(n, 0.25)


def impulse_pair(n):
    x = np.zeros(n)
    x[0] = 0.7
    x[n - 1] = -0.7
    return x


def sentinel(n, peak):
    """A frame whose 4x peak is `peak` (0.9e-10 / 1.1e-10) and lies on phase 2, so that 1x stays below
    the threshold either way."""
    return pulse(n, n // 3 + 0.5, peak)


@functools.lru_cache(maxsize=None)
def designed(n):
    """All designed frames of length n: ([name...], float32 [F, n]). Neighbouring frames win on different
    phases. The tuple (kind, winning phase or None) is part of the name list for the CPU property test."""
    out = []
    if n >= 16:
        for where, c0 in (("mid", n // 3), ("wrap0", 0), ("wrapN", n - 1)):
            for p in (1, 2, 3):
                out.append((f"pulse_{where}_p{p}", "pulse", p, pulse(n, c0 + p / 4.0)))
        if n % 4 == 0:
            for p in (1, 2, 3):
                out.append((f"tone_p{p}", "tone", p, tone(n, p)))
    if n % 2 == 0:
        out.append(("nyquist", "nyquist", 0, nyquist(n)))
        if n >= 16:
            out.append(("nyqmix_pulse_p1", "nyqmix", 1, nyquist_mix_pulse(n, 1)))
            out.append(("nyqmix_pulse_p3", "nyqmix", 3, nyquist_mix_pulse(n, 3)))
            if n % 4 == 0:
                out.append(("nyqmix_tone_p1", "nyqmix", 1, nyquist_mix_tone(n, 1)))
                out.append(("nyqmix_tone_p3", "nyqmix", 3, nyquist_mix_tone(n, 3)))
    out.append(("dc", "dc", None, dc(n)))
    out.append(("impulse_pair", "edge", None, impulse_pair(n)))
    out.append(("below_silence", "sentinel", None, sentinel(n, 0.9e-10)))
    out.append(("above_silence", "sentinel", None, sentinel(n, 1.1e-10)))
    names = [o[0] for o in out]
    meta = {o[0]: (o[1], o[2]) for o in out}
    frames = np.stack([o[3] for o in out]).astype(np.float32)
    frames.setflags(write=False)
    return names, meta, frames


@functools.lru_cache(maxsize=None)
def reference(n):
    """float64 per-phase maxima [F, 4] of designed(n)'s float32 frames (computed once per length)."""
    _, _, frames = designed(n)
    ph = np.stack([phase_peaks(f) for f in frames])
    ph.setflags(write=False)
    return ph
