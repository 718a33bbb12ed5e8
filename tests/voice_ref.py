"""The voice-detection device row restated in numpy and scipy (TEST INFRASTRUCTURE ONLY): what
omega_voice_features writes per frame, from the reference's own expressions
(omega4/panels/voice_detection.py:57-122 and :169-192). tests/golden/gen_voice.py asserts it equal to the
reference's results; tests/test_voice.py pins it to the golden bit for bit and feeds its rows to the facade's
host logic.

The row differs from the reference's intermediate values in one respect: voice_energy and total_energy are
float64 sums of the float32 bins (the reference's are numpy's float32 pairwise sums); the facade rounds them
to float32 before it forms the ratio. Float32 audio is widened to float64 first, as the device does.
"""
import numpy as np
from scipy import signal

COLUMNS = ("flags", "voice_start", "voice_end", "voice_energy", "total_energy", "formant_count",
           "f1_bin", "f2_bin", "f3_bin", "f4_bin", "f1_freq", "f2_freq", "f3_freq", "f4_freq",
           "corr0", "peak_lag", "corr_peak")
FLAG_RANGE, FLAG_NO_ENERGY, FLAG_NONFINITE, FLAG_NO_PITCH = 1, 2, 4, 8
FORMANT_RANGES = ((200, 900), (800, 2500), (2000, 3500), (3000, 4500))


def bin_range(fs, m):
    """:64-67."""
    fb = np.fft.rfftfreq(m, 1 / fs)
    return int(np.searchsorted(fb, 85)), int(np.searchsorted(fb, 255))


def has_pitch(fs, m):
    """:174, :185: the shape can give a pitch at all."""
    return m >= 2048 and int(fs / 80) < m


def smoothed_peaks(spectrum):
    """:97-98: (smoothed float32, kept peaks, their prominences, the threshold); None for len <= 10."""
    spectrum = np.asarray(spectrum, np.float32)
    if len(spectrum) <= 10:
        return None
    sm = signal.savgol_filter(spectrum, min(11, len(spectrum) // 4 * 2 + 1), 3)
    thr = np.max(sm) * 0.1
    peaks, props = signal.find_peaks(sm, prominence=thr)
    return sm, peaks, props["prominences"], thr


def formants(spectrum, fs, m):
    """:101-115 per range: (bin, freq) of its first kept peak, or None."""
    sp = smoothed_peaks(spectrum)
    fb = np.fft.rfftfreq(m, 1 / fs)
    out = [None] * 4
    if sp is None:
        return out
    for r, (lo, hi) in enumerate(FORMANT_RANGES):
        for peak in sp[1]:
            if peak < len(fb) and lo <= fb[peak] <= hi:
                out[r] = (int(peak), fb[peak])
                break
    return out


def autocorr(audio, fs):
    """:178-188 on float64: (corr0, peak_lag, corr_peak)."""
    x = np.asarray(audio, np.float64)
    corr = np.correlate(x, x, mode="full")
    corr = corr[len(corr) // 2:]
    lo, hi = int(fs / 400), int(fs / 80)
    lag = int(np.argmax(corr[lo:hi])) + lo
    return corr[0], lag, corr[lag]


def row(spectrum, audio, fs):
    spectrum = np.asarray(spectrum, np.float32)
    K, m = len(spectrum), len(audio)
    pitch = has_pitch(fs, m)
    out = np.zeros(len(COLUMNS), np.float64)
    if not np.all(np.isfinite(spectrum)) or (pitch and not np.all(np.isfinite(audio))):
        out[0] = FLAG_NONFINITE
        return out
    flags = 0 if pitch else FLAG_NO_PITCH
    vs, ve = bin_range(fs, m)
    out[1], out[2] = vs, ve
    if pitch:
        out[14:17] = autocorr(audio, fs)
    if not (vs < K and ve < K):
        out[0] = flags | FLAG_RANGE
        return out
    out[3] = np.sum(spectrum[vs:ve], dtype=np.float64)
    out[4] = np.sum(spectrum, dtype=np.float64)
    if not out[4] > 0:
        out[0] = flags | FLAG_NO_ENERGY
        return out
    out[0] = flags
    for r, f in enumerate(formants(spectrum, fs, m)):
        if f is not None:
            out[5] += 1
            out[6 + r], out[10 + r] = f
    return out
