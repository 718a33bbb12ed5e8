"""numpy/scipy restatement of CepstralAnalyzer (omega4/panels/pitch_detection.py:21-611) for the pitch
tests. TEST INFRASTRUCTURE ONLY: the product (csrc/pitch.hip, omega_gpu/pitch_detection.py) does not
import it and does not depend on scipy.

``analyze(x, P)`` returns every intermediate decision of one detect_pitch_advanced call (:485-556):
the integer cepstral period, autocorrelation period and YIN tau beside the (pitch, confidence) pairs
and the combined result. ``f64=True`` evaluates the float32 paths (autocorrelation :176-227, YIN
:229-316) with the same formulas in float64 -- the yardstick the float32-path tolerances of
tests/test_pitch.py are measured against.
"""
from __future__ import annotations

from collections import deque

import numpy as np
from scipy import signal as sps

NOTE_NAMES = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]


class Params:
    """The fields detect_pitch_advanced reads (:24-44 and pitch_detection_config.py:104-121)."""

    def __init__(self, sample_rate=48000, min_pitch=50.0, max_pitch=2000.0, yin_threshold=0.15, yin_window_size=1920,
                 enable_preprocessing=True, highpass_frequency=80.0, highpass_order=4, enable_compression=True,
                 compression_threshold=0.1, compression_ratio=0.5):
        self.sample_rate = sample_rate
        self.min_pitch, self.max_pitch = min_pitch, max_pitch
        self.min_period = int(sample_rate / max_pitch)  # :35
        self.max_period = int(sample_rate / min_pitch)  # :36
        self.yin_threshold, self.yin_window_size = yin_threshold, yin_window_size
        self.enable_preprocessing = enable_preprocessing
        self.highpass_frequency, self.highpass_order = highpass_frequency, highpass_order
        self.enable_compression = enable_compression
        self.compression_threshold, self.compression_ratio = compression_threshold, compression_ratio

    @classmethod
    def from_config(cls, cfg):
        return cls(cfg.sample_rate, cfg.min_pitch, cfg.max_pitch, cfg.yin_threshold, cfg.yin_window_size,
                   cfg.enable_preprocessing, cfg.highpass_frequency, cfg.highpass_order, cfg.enable_compression,
                   cfg.compression_threshold, cfg.compression_ratio)


def preprocess(x, P):
    """:497-525: float64 high-pass cascade (sosfilt promotes), RMS compression / the quiet branch."""
    if not P.enable_preprocessing:
        return x
    sos = sps.butter(P.highpass_order, P.highpass_frequency / (P.sample_rate / 2), btype="high", output="sos")
    f = sps.sosfilt(sos, x)
    if P.enable_compression:
        rms = np.sqrt(np.mean(f ** 2))
        if rms > 0.01 and rms > P.compression_threshold:
            gain = P.compression_threshold + (rms - P.compression_threshold) * P.compression_ratio
            f = f * (gain / rms)
    elif np.sqrt(np.mean(f ** 2)) < 0.01:
        f = x
    return f


def cepstrum(f):
    """:132-144"""
    spec = np.fft.rfft(f * np.hanning(len(f)))
    c = np.fft.irfft(np.log(np.abs(spec) + 1e-10))
    return c[:len(c) // 2]


def pick_cepstral(c, P):
    """:146-174 -> (period, pitch, confidence); period 0: no estimate."""
    lo, hi = P.min_period, min(P.max_period, len(c) - 1)
    if hi <= lo:
        return 0, 0.0, 0.0
    v = c[lo:hi]
    peaks, prop = sps.find_peaks(v, height=np.max(v) * 0.3, distance=20)
    if len(peaks) == 0:
        return 0, 0.0, 0.0
    k = int(np.argmax(prop["peak_heights"]))
    period = int(peaks[k]) + lo
    return period, P.sample_rate / period, min(1.0, prop["peak_heights"][k] / np.std(c))


def autocorrelation(x, f64=False):
    """:176-195 (float32 in, float32 out with numpy >= 2; f64: the same in float64)."""
    if f64:
        x = x.astype(np.float64)
    x = x - np.mean(x)
    n = len(x)
    size = 2 ** int(np.ceil(np.log2(2 * n - 1)))
    F = np.fft.rfft(x, size)
    r = np.fft.irfft(F * np.conj(F))[:n]
    return r / (r[0] + 1e-10)


def pick_autocorr(r, P):
    """:197-227 -> (period, pitch, confidence, first raw local maximum >= 0.3 or 0)."""
    lo, hi = P.min_period, min(P.max_period, len(r) - 1)
    if hi <= lo:
        return 0, 0.0, 0.0, 0
    v = r[lo:hi]
    peaks, _ = sps.find_peaks(v, height=0.3, distance=20)
    raw, _ = sps.find_peaks(v, height=0.3)
    first_raw = int(raw[0]) + lo if len(raw) else 0
    if len(peaks) == 0:
        return 0, 0.0, 0.0, first_raw
    period = int(peaks[0]) + lo
    return period, P.sample_rate / period, r[period], first_raw


def yin_cmnd(x, P, f64=False):
    """:245-277: the difference function in both of its definitions and the cumulative mean
    normalised difference. f64: direct float64 sums (the three-dot form equals the zero-padded
    squared-difference sum exactly)."""
    n = len(x)
    max_tau = min(P.max_period, n // 2)
    d = np.zeros(max_tau)
    small = min(100, max_tau)
    if f64:
        x = x.astype(np.float64)
        xp = np.pad(x, (0, max_tau))
        for tau in range(1, small):
            d[tau] = np.sum((x[:-tau] - x[tau:]) ** 2)
        for tau in range(small, max_tau):
            d[tau] = np.sum((x - xp[tau:tau + n]) ** 2)
    else:
        for tau in range(1, small):
            d[tau] = np.sum((x[:-tau] - x[tau:]) ** 2)
        xp = np.pad(x, (0, max_tau), mode="constant")
        for tau in range(small, max_tau):
            s = xp[tau:tau + n]
            d[tau] = np.dot(x, x) + np.dot(s, s) - 2 * np.dot(x, s)
    cm = np.ones(max_tau)
    cs = np.cumsum(d)
    cm[1:] = d[1:] * np.arange(1, max_tau) / cs[1:]
    return cm, max_tau


def pick_yin(cm, max_tau, P):
    """:279-316, :363-371 -> (tau, pitch, confidence)."""
    tau = 0
    for t in range(P.min_period, max_tau - 1):
        if cm[t] < P.yin_threshold and cm[t] < cm[t - 1] and cm[t] < cm[t + 1]:
            tau = t
            break
    if tau == 0:
        return 0, 0.0, 0.0
    a = (cm[tau - 1] - 2 * cm[tau] + cm[tau + 1]) / 2
    b = (cm[tau + 1] - cm[tau - 1]) / 2
    tf = tau + (-b / (2 * a)) if a != 0 else float(tau)
    return tau, P.sample_rate / tf, 1.0 - cm[tau]


def combine(methods, P):
    """:384-433 with its hard-coded thresholds and weights -> (pitch, confidence, std/mean or nan)."""
    (cp, cc), (ap, ac), (yp, yc) = methods
    est = []
    if cc > 0.15 and P.min_pitch <= cp <= P.max_pitch:
        est.append((cp, cc * 0.8))
    if ac > 0.2 and P.min_pitch <= ap <= P.max_pitch:
        est.append((ap, ac * 0.9))
    if yc > 0.25 and P.min_pitch <= yp <= P.max_pitch:
        est.append((yp, yc * 1.1))
    if not est:
        return 0.0, 0.0, float("nan")
    tw = sum(c for _, c in est)
    pitch = sum(p * c for p, c in est) / tw
    conf = tw / len(est)
    ratio = float("nan")
    if len(est) >= 2:
        ps = [p for p, _ in est]
        ratio = np.std(ps) / np.mean(ps)
        if ratio < 0.02:
            conf = min(1.0, conf * 1.2)
        elif ratio > 0.05:
            conf *= 0.8
    return pitch, conf, ratio


def pitch_to_note(pitch):
    """:435-456 -> (note, octave, cents, the unrounded cents value)."""
    if pitch <= 0:
        return "", 0, 0, 0.0
    c0 = 440.0 * (2 ** (-4.75))
    semis = 12 * np.log2(pitch / c0)
    r = int(round(semis))
    cents = (semis - r) * 100
    return NOTE_NAMES[r % 12], r // 12, int(cents), float(cents)


def stability(pitches, confidences):
    """:458-483 over the two histories."""
    if len(pitches) < 10:
        return 0.0
    rp, rc = list(pitches)[-20:], list(confidences)[-20:]
    valid = [p for p, c in zip(rp, rc) if c > 0.3 and p > 0]
    if len(valid) < 5:
        return 0.0
    m, s = np.mean(valid), np.std(valid)
    return max(0.0, 1.0 - (s / m) * 10) if m > 0 else 0.0


def analyze(x, P, f64=False):
    """One detect_pitch_advanced call on a float32 frame of at least yin_window_size samples."""
    x = np.asarray(x, np.float32)
    c = cepstrum(preprocess(x, P))
    cper, cp, cc = pick_cepstral(c, P)
    aper, ap, ac, first_raw = pick_autocorr(autocorrelation(x, f64), P)
    cm, max_tau = yin_cmnd(x[:P.yin_window_size], P, f64)
    tau, yp, yc = pick_yin(cm, max_tau, P)
    pitch, conf, ratio = combine(((cp, cc), (ap, ac), (yp, yc)), P)
    note, octave, cents, cents_f = pitch_to_note(pitch)
    return dict(cep_period=cper, ac_period=aper, yin_tau=tau, ac_first_raw=first_raw,
                cepstral=(cp, cc), autocorr=(ap, ac), yin=(yp, yc), pitch=pitch, confidence=conf, ratio=ratio,
                note=note, octave=octave, cents_offset=cents, cents_float=cents_f)


class Analyzer:
    """The stateful part (:46-48, :538-546): histories and stability over analyze()."""

    def __init__(self, P, max_history_length=100):
        self.P = P
        self.pitch_history = deque(maxlen=max_history_length)
        self.confidence_history = deque(maxlen=max_history_length)

    def detect(self, x):
        r = analyze(x, self.P)
        self.pitch_history.append(r["pitch"])
        self.confidence_history.append(r["confidence"])
        r["stability"] = stability(self.pitch_history, self.confidence_history)
        return r
