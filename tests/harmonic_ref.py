"""numpy/scipy restatement of HarmonicAnalyzer.detect_harmonic_series
(omega4/panels/harmonic_analysis.py:193-333) and the HarmonicMetrics it calls
(omega4/analyzers/harmonic_metrics.py:51-357) for the harmonic tests. TEST INFRASTRUCTURE ONLY: the
product (csrc/harmonic.hip, omega_gpu/harmonic_analysis.py) does not import it and does not depend on
scipy.

``analyze(spec, freqs, audio, fs, prev)`` returns every intermediate decision of one call -- the peaks
find_peaks keeps, per kept series the peak bin, the accepted harmonic bins and the strength, the
rolloff index, the LPC lags, coefficients and roots -- beside the result values. The spectrum is taken
as float32, like the app's, and numpy's scalar promotion (NEP 50) then keeps the float32 paths in
float32 exactly as in the reference; ``f64=True`` widens the spectrum first, which evaluates every one
of those formulas in float64 -- the yardstick the float32-path tolerances of tests/test_harmonic.py are
measured against. ``formants_ext`` is the extended-precision evaluation of the formant path
(np.longdouble lags and recursion, the roots polished by Newton steps in longdouble).
"""
from __future__ import annotations

import numpy as np
from scipy import signal as sps

MAX_HARMONIC = 16
ORDER = 14
REAL_ROOT = 1e-8  # csrc/harmonic.hip: |imag| <= 1e-8 max(1, |z|) is a real root


CHECKS = None  # a list while tests/golden/gen_harmonic.py records: (kind, margin) of every decision taken


def note(kind, margin):
    if CHECKS is not None:
        CHECKS.append((kind, float(margin)))


def nearest(freqs, target):
    d = np.abs(freqs - target)
    i = int(np.argmin(d))
    if CHECKS is not None:
        two = np.partition(d, 1)[:2]
        note("argmin", (two[1] - two[0]) / (freqs[1] - freqs[0]))
    return i


def series_from(x, freqs, peak, nyquist):
    """:281-333 for the fundamental at bin `peak`: (bins[16] with -1 = not accepted, strength, count)."""
    f0, fmag = freqs[peak], x[peak]
    bins = np.full(MAX_HARMONIC, -1, np.int32)
    rel = {}
    for n in range(1, MAX_HARMONIC + 1):
        hf = f0 * n
        if hf > nyquist:
            break
        i = nearest(freqs, hf)
        note("tol5", abs(abs(freqs[i] - hf) - f0 * 0.05) / f0)
        if abs(freqs[i] - hf) <= f0 * 0.05:
            bins[n - 1] = i
            rel[n] = x[i] / (fmag + 1e-10)
    strength = 0.0
    if len(rel) >= 2:
        for n in sorted(rel)[:8]:
            strength = strength + rel[n] * (1.0 / n)
        strength = strength / sum(1.0 / n for n in range(1, min(9, len(rel) + 1)))
    return bins, strength, len(rel)


def thd(x, freqs, f0, nyquist):
    if f0 <= 0 or f0 > nyquist:
        return 0.0
    fp = x[nearest(freqs, f0)] ** 2
    note("fund_power", abs(float(fp) - 1e-10) / 1e-10)
    if fp < 1e-10:
        return 0.0
    hs = 0.0
    for n in range(2, 6):
        if f0 * n > nyquist:
            break
        i = nearest(freqs, f0 * n)
        note("tol10", abs(abs(freqs[i] - f0 * n) - f0 * 0.1) / f0)
        if abs(freqs[i] - f0 * n) < f0 * 0.1:
            hs = hs + x[i] ** 2
    return min(np.sqrt(hs / fp) * 100, 100.0)


def thd_plus_noise(x, freqs, f0, nyquist):
    if f0 <= 0 or f0 > nyquist:
        return 0.0
    fp = x[nearest(freqs, f0)] ** 2
    if fp < 1e-10:
        return 0.0
    a, b = nearest(freqs, f0 - f0 * 0.05), nearest(freqs, f0 + f0 * 0.05)
    rest = np.sum(x ** 2) - np.sum(x[a:b + 1] ** 2)
    return min(np.sqrt(rest / fp) * 100, 100.0)


def centroid_spread_rolloff(x, freqs):
    mag = np.abs(x)
    tot = np.sum(mag)
    if not tot > 0:
        return 0.0, 0.0, 0.0, -1
    c = np.sum(freqs * mag) / tot
    sp = np.sqrt(np.sum(((freqs - c) ** 2) * mag) / tot)
    cs = np.cumsum(mag)
    idx = int(np.nonzero(cs >= 0.85 * cs[-1])[0][0])
    return c, sp, freqs[idx], idx


def rolloff_margin(x):
    """How far (relative to the total) the cumulative magnitude is from the 85 % threshold either side of the decision."""
    cs = np.cumsum(np.abs(x.astype(np.float64)))
    thr = 0.85 * cs[-1]
    i = int(np.nonzero(cs >= thr)[0][0])
    lo = thr - cs[i - 1] if i > 0 else np.inf
    return float(min(cs[i] - thr, lo) / cs[-1])


def flux(x, prev):
    n = min(len(x), len(prev))
    return np.sum(np.maximum(np.abs(x[:n]) - np.abs(prev[:n]), 0))


def inharmonicity(x, freqs, f0, nyquist):
    devs = []
    for n in range(2, 11):
        ef = f0 * n
        if ef > nyquist:
            break
        a, b = nearest(freqs, ef - f0 * 0.1), nearest(freqs, ef + f0 * 0.1)
        if b > a:
            if CHECKS is not None and b - a > 1:
                top = np.sort(x[a:b].astype(np.float64))[-2:]
                note("argmax", (top[1] - top[0]) / max(top[1], 1e-30))
            devs.append(abs(freqs[a + int(np.argmax(x[a:b]))] - ef) / ef)
    return np.mean(devs) if devs else 0.0


def hnr(x, freqs, f0, nyquist):
    mask = np.zeros(len(x), bool)
    he = 0.0
    for n in range(1, 6):
        if f0 * n > nyquist:
            break
        i = nearest(freqs, f0 * n)
        if abs(freqs[i] - f0 * n) < f0 * 0.1:
            he = he + x[i] ** 2
            bw = int(f0 * 0.05 / (freqs[1] - freqs[0]))
            mask[max(0, i - bw):min(len(x), i + bw + 1)] = True
    rest = x[~mask] ** 2
    ne = np.cumsum(rest)[-1] if len(rest) else 0.0  # (a running sum in the spectrum's precision)
    if ne > 0:
        with np.errstate(divide="ignore"):
            return max(0, min(10 * np.log10(he / ne), 60))
    return 60.0


def lpc(audio, ld=False):
    """:115-196 up to the polynomial: (lags[15], coefficients[15] of z^14 ... z^0) or None (no formants)."""
    T = np.longdouble if ld else np.float64
    x = np.asarray(audio).astype(T)
    m = len(x)
    if m < ORDER + 1 or np.max(np.abs(x)) < 1e-10:
        return None
    e = np.concatenate([x[:1], x[1:] - T(0.97) * x[:-1]])
    if ld:
        k = np.arange(1 - m, m, 2).astype(T)
        win = T("0.54") + T("0.46") * np.cos(T("3.14159265358979323846264338327950288") * k / (m - 1))
    else:
        win = np.hamming(m)
    w = e * win
    r = np.array([np.dot(w[:m - k], w[k:]) for k in range(ORDER + 1)], T)
    if abs(r[0]) < 1e-10:
        return None
    a = np.zeros(ORDER + 1, T)
    a[0] = 1
    for q in range(ORDER):
        if q == 0:
            km = -r[1] / r[0]
        else:  # term by term, like the reference (a dot product may round differently)
            s = T(0)
            for j in range(q + 1):
                s = s + a[j] * r[q - j]
            km = -s / r[0]
        nxt = a.copy()
        for i in range(1, q + 2):
            nxt[i] = a[i] + km * a[q + 1 - i]
        a = nxt
    return r, a


def formants_from_roots(roots, fs, real_tol=0.0):
    out = []
    for z in roots:
        if z.imag > real_tol * max(1.0, abs(z)):
            fq = float(np.angle(complex(z))) * fs / (2 * np.pi)
            if 50 < fq < fs / 2:
                out.append(fq)
    return sorted(out)[:4]


def formants(audio, fs):
    """-> (formants, lags, roots); ([], None, None) where the reference returns early."""
    got = lpc(audio)
    if got is None:
        return [], None, None
    r, a = got
    roots = np.roots(a)
    return formants_from_roots(roots, fs), r, roots


def formants_ext(audio, fs):
    """The formants from longdouble lags and recursion, roots polished in longdouble: (formants, roots)."""
    got = lpc(audio, ld=True)
    if got is None:
        return [], None
    _, a = got
    z = np.roots(a.astype(np.float64)).astype(np.clongdouble)
    da = a[:-1] * np.arange(ORDER, 0, -1).astype(np.longdouble)
    for _ in range(8):
        p = np.zeros_like(z) + a[0]
        for c in a[1:]:
            p = p * z + c
        d = np.zeros_like(z) + da[0]
        for c in da[1:]:
            d = d * z + c
        z = z - p / d
    out = []
    for v in z:
        if v.imag > REAL_ROOT * max(1.0, abs(v)):
            fq = np.arctan2(v.imag, v.real) * fs / (2 * np.longdouble("3.14159265358979323846264338327950288"))
            if 50 < fq < fs / 2:
                out.append(float(fq))
    return sorted(out)[:4], z


def analyze(spec, freqs, audio=None, fs=48000, prev=None, f64=False, select=None):
    """One detect_harmonic_series call. prev: the previous call's spectrum or None. select: None for scipy's
    own distance rule, or select(x, candidates, distance) -> the kept peaks (the rule of
    tools/model/peaks_model.py, for spectra with equal heights where scipy has no rule of its own)."""
    x = np.asarray(spec, np.float32)
    if f64:
        x = x.astype(np.float64)
        prev = None if prev is None else np.asarray(prev, np.float32).astype(np.float64)
    freqs = np.asarray(freqs, np.float64)
    nyq = fs / 2
    peaks, _ = sps.find_peaks(x, height=np.max(x) * 0.1, distance=10)
    if select is not None:  # find_peaks' order: the height condition, then the distance rule
        peaks = np.asarray(select(x, list(sps.find_peaks(x, height=np.max(x) * 0.1)[0]), 10), np.intp)
    found = []
    for pk in peaks:
        if 20 <= freqs[pk] <= 2000:
            bins, s, cnt = series_from(x, freqs, int(pk), nyq)
            if s > 0.3:
                found.append((int(pk), bins, s, cnt))
    cand = [(int(pk), series_from(x, freqs, int(pk), nyq)[1]) for pk in peaks if 20 <= freqs[pk] <= 2000]
    found.sort(key=lambda e: e[2], reverse=True)
    r = dict(peaks=np.asarray(peaks, np.int32), candidates=cand, series_peak=np.array([e[0] for e in found], np.int32),
             series_bins=np.array([e[1] for e in found], np.int32).reshape(-1, MAX_HARMONIC),
             series_strength=np.array([e[2] for e in found], np.float64), series_count=len(found),
             dominant_fundamental=0.0, thd=0.0, thd_plus_noise=0.0, spectral_centroid=0.0, spectral_spread=0.0,
             spectral_flux=0.0, spectral_rolloff=0.0, rolloff_idx=-1, inharmonicity=0.0, hnr_db=0.0, formants=[],
             lags=None, roots=None)
    if found:
        f0 = freqs[found[0][0]]
        c, sp, ro, ri = centroid_spread_rolloff(x, freqs)
        r.update(dominant_fundamental=float(f0), thd=float(thd(x, freqs, f0, nyq)),
                 thd_plus_noise=float(thd_plus_noise(x, freqs, f0, nyq)), spectral_centroid=float(c),
                 spectral_spread=float(sp), spectral_rolloff=float(ro), rolloff_idx=ri,
                 spectral_flux=float(flux(x, prev)) if prev is not None else 0.0,
                 inharmonicity=float(inharmonicity(x, freqs, f0, nyq)), hnr_db=float(hnr(x, freqs, f0, nyq)))
        if audio is not None and len(audio) > ORDER:
            r["formants"], r["lags"], r["roots"] = formants(audio, fs)
    return r


def row(r):
    """The result as omega_harmonic_analyze's first 15 columns."""
    fm = list(r["formants"])
    return np.array([r["series_count"], r["dominant_fundamental"], r["thd"], r["thd_plus_noise"], r["spectral_centroid"],
                     r["spectral_spread"], r["spectral_flux"], r["spectral_rolloff"], r["inharmonicity"], r["hnr_db"],
                     len(fm)] + fm + [0.0] * (4 - len(fm)), np.float64)
