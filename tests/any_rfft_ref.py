"""Designed signals and the float64 expectation of the any-length windowed rfft (anyfft.hip,
any_rfft_kernel) for tests/test_any_rfft.py. TEST INFRASTRUCTURE ONLY: the product does not import it.

``designed(n, window)`` returns named float32 frames, each built so that one kind of defect shows in single
bins and not only in a norm, with the closed form of the windowed spectrum where one exists:

  impulse_d  unit impulse at d in {0, 1, n//3, n-1}: X_k = w[d] e^{-2 pi i k d / n}; with the rectangular
             window every bin has magnitude 1, so an error relative to max |X| is a per-bin relative error
             and a misplaced output or a wrong twiddle power turns one or more phases
  tone_k0    cos(2 pi k0 i / n + 0.3), k0 in {1, n//4 or 1, (n-1)//2}: the energy sits in one bin (leakage
             everywhere else); rect: X_k = (n/2) (e^{0.3i} [k = k0 mod n] + e^{-0.3i} [k = -k0 mod n])
  nyquist    (-1)^i (even n), and dc (0.25): the tiny lengths 1 and 2 reduce to these
  ramp       i / n - 0.5: not symmetric, catches conjugate or reversed-order errors
  noise      oracle.signals.noise(4, n, 0.2), the signal of test_gpu_parity.py's any-length lines

``expect(frame, window)`` is np.fft.rfft of the float64 product of the float32 frame and the float32 window
the oracle uses (oracle.omega_ref.window_f32): the device multiplies float32 by that same float32 window,
so the window's own rounding is not counted against it. ``yardstick(frame, window)`` is the reference's own
float32 path (oracle.omega_ref.gpu_fft; np.fft.rfft of the float32 product for `rect`), complex64, and
``deviation`` its distance from ``expect``: max_k |X32 - X64| / max_k |X64|.

``designed_pow2`` / ``reference_pow2`` are the same for tests/test_pow2_rfft_bins.py, with the tones and the
two-impulse frame the power-of-two kernels need on top (see there).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import omega_ref as R
from oracle import signals as S

WINDOWS = ("rect", "hann", "hamming", "blackman")
PHI = 0.3
NOISE_SEED = 4


def window64(n, window):
    """The oracle's float32 window (np.hanning / np.hamming / np.blackman(n).astype(float32), ones for
    `rect`) as float64."""
    assert window in WINDOWS
    return np.asarray(R.window_f32(n, window), np.float64)


def impulse_positions(n):
    return sorted({0, 1 % n, n // 3, n - 1})


def tone_bins(n):
    return sorted({1, n // 4 or 1, (n - 1) // 2})


def impulse(n, d):
    x = np.zeros(n)
    x[d] = 1.0
    return x


def tone(n, k0):
    return np.cos(2 * np.pi * ((k0 * np.arange(n)) % n) / n + PHI)  # (the argument reduced exactly)


def nyquist(n):
    assert n % 2 == 0
    return np.where(np.arange(n) % 2 == 0, 1.0, -1.0)


def dc(n):
    return np.full(n, 0.25)


def ramp(n):
    return np.arange(n, dtype=np.float64) / n - 0.5


def signals64(n):
    """[(name, float64 frame)] before the cast to float32."""
    out = [(f"impulse_{d}", impulse(n, d)) for d in impulse_positions(n)]
    out += [(f"tone_{k0}", tone(n, k0)) for k0 in tone_bins(n)]
    if n % 2 == 0:
        out.append(("nyquist", nyquist(n)))
    out.append(("dc", dc(n)))
    out.append(("ramp", ramp(n)))
    out.append(("noise", S.noise(NOISE_SEED, n, 0.2).astype(np.float64)))
    return out


def closed_form(name, n, window):
    """The windowed spectrum [n//2 + 1] of the float64 signal `name` in closed form, or None."""
    k = np.arange(n // 2 + 1)
    kind, _, arg = name.partition("_")
    if kind == "impulse":
        d = int(arg)
        return window64(n, window)[d] * np.exp(-2j * np.pi * ((k * d) % n) / n)
    if window != "rect":
        return None
    X = np.zeros(n // 2 + 1, np.complex128)
    if kind == "dc":
        X[0] = 0.25 * n
    elif kind == "nyquist":
        X[n // 2] = n
    elif kind == "tone":
        k0 = int(arg)
        X[k == k0 % n] += 0.5 * n * np.exp(1j * PHI)
        X[k == (-k0) % n] += 0.5 * n * np.exp(-1j * PHI)
    else:
        return None
    return X


@functools.lru_cache(maxsize=None)
def designed(n, window="rect"):
    """All designed frames of length n: ([name...], {name: closed form under `window` or None}, float32
    [F, n]). The frames are the same for every window; the closed forms are not."""
    sig = signals64(n)
    names = [s[0] for s in sig]
    closed = {nm: closed_form(nm, n, window) for nm in names}
    frames = np.stack([s[1] for s in sig]).astype(np.float32)
    frames.setflags(write=False)
    return names, closed, frames


def expect(frame, window):
    """np.fft.rfft(float64(frame) * float64(float32 window)), complex128."""
    frame = np.asarray(frame)
    return np.fft.rfft(frame.astype(np.float64) * window64(len(frame), window))


def yardstick(frame, window):
    """The reference's float32 path on the float32 frame, complex64."""
    frame = np.asarray(frame)
    assert frame.dtype == np.float32
    if window == "rect":
        X = np.fft.rfft(frame * R.window_f32(len(frame), "rect"))
    else:
        X = R.gpu_fft(frame, window)[1]
    assert X.dtype == np.complex64, X.dtype
    return X


def deviation(X32, X64):
    """max_k |X32 - X64| / max_k |X64| (0 for an all-zero expectation met exactly)."""
    X64 = np.asarray(X64, np.complex128)
    den = float(np.max(np.abs(X64)))
    num = float(np.max(np.abs(np.asarray(X32).astype(np.complex128) - X64)))
    if den == 0.0:
        assert num == 0.0
        return 0.0
    return num / den


@functools.lru_cache(maxsize=None)
def reference(n, window):
    """(X64 [F, n//2 + 1] complex128, dev [F]) of designed(n)'s frames under `window`, computed once."""
    _, _, frames = designed(n, window)
    X = np.stack([expect(f, window) for f in frames])
    dev = np.array([deviation(yardstick(f, window), x) for f, x in zip(frames, X)])
    X.setflags(write=False)
    dev.setflags(write=False)
    return X, dev


# ---- additions for the power-of-two kernels (tests/test_pow2_rfft_bins.py) ----

REG_FFT_MIN = 8192  # the register FFT (regfft.hpp RegFFT<K>, K = n / 2 = 4096, 8192) serves these lengths
PAIR_LEVEL = 0.5


def pow2_tone_bins(n):
    """On-bin tones beyond tone_bins(n) for n = 2K a power of two: the special slots of untangle and
    rfft_magnitudes (bins 1, K/2 - 1, K/2, K/2 + 1, K - 1) and, where the register FFT runs (n >= 8192,
    NTH = K / 16 threads, thread t owning the bins t + NTH q), the bins t + NTH q for q in {0, 7} and
    t in {0, 63, 64, 255}: wave and round edges of the pair ownership. Bins past n / 2 or below 0 (tiny
    n) are dropped, as are those tone_bins(n) already has."""
    assert n >= 2 and n & (n - 1) == 0
    K = n // 2
    bins = {1, K // 2 - 1, K // 2, K // 2 + 1, K - 1}
    if n >= REG_FFT_MIN:
        nth = K // 16
        bins |= {t + nth * q for q in (0, 7) for t in (0, 63, 64, 255)}
    return sorted(b for b in bins if 0 <= b <= K and b not in tone_bins(n))


def pair_positions(n):
    """(a, b) of the `pair` frame: a = n // 3, b = a + an odd distance near n / 6."""
    a = n // 3
    return a, a + ((n // 6) | 1)


def pair(n):
    """Unit impulse at a plus PAIR_LEVEL at b: |X_k| = |w[a] + PAIR_LEVEL w[b] e^{-2 pi i k (b - a) / n}|
    differs from bin to bin (between 0.5 and 1.5 under `rect`) and, b - a being odd, between k and
    n / 2 - k: it tells the bins apart for the paths that emit magnitudes only, on which a single impulse
    has the same magnitude in every bin."""
    a, b = pair_positions(n)
    assert a < b < n
    x = np.zeros(n)
    x[a] = 1.0
    x[b] = PAIR_LEVEL
    return x


def pow2_signals64(n):
    """signals64(n), the further tones of pow2_tone_bins(n) and the `pair` frame."""
    out = signals64(n)
    out += [(f"tone_{k0}", tone(n, k0)) for k0 in pow2_tone_bins(n)]
    out.append(("pair", pair(n)))
    return out


def pow2_closed_form(name, n, window):
    if name == "pair":
        a, b = pair_positions(n)
        k = np.arange(n // 2 + 1)
        w = window64(n, window)
        return w[a] * np.exp(-2j * np.pi * ((k * a) % n) / n) + PAIR_LEVEL * w[b] * np.exp(-2j * np.pi * ((k * b) % n) / n)
    return closed_form(name, n, window)  # (tone_0 and a tone at n / 2: both exponentials land on one bin)


@functools.lru_cache(maxsize=None)
def designed_pow2(n, window="rect"):
    """designed(n, window) over pow2_signals64(n): ([name...], {name: closed form or None}, float32 [F, n])."""
    sig = pow2_signals64(n)
    names = [s[0] for s in sig]
    assert len(set(names)) == len(names)
    closed = {nm: pow2_closed_form(nm, n, window) for nm in names}
    frames = np.stack([s[1] for s in sig]).astype(np.float32)
    frames.setflags(write=False)
    return names, closed, frames


@functools.lru_cache(maxsize=None)
def reference_pow2(n, window):
    """(X64 [F, n//2 + 1] complex128, dev [F]) of designed_pow2(n)'s frames under `window`, computed once
    (dev = 0 for a frame whose windowed product is exactly zero)."""
    _, _, frames = designed_pow2(n, window)
    X = np.stack([expect(f, window) for f in frames])
    dev = np.array([deviation(yardstick(f, window), x) for f, x in zip(frames, X)])
    X.setflags(write=False)
    dev.setflags(write=False)
    return X, dev


# ---- the transform of anyfft.hip's header comment, restated ----

def fft_radices(n):
    """design.cpp fft_radices: 4s, then 2, 3, 5, 7, then the remaining primes in ascending order."""
    rad, r = [], n
    while r % 4 == 0:
        rad.append(4)
        r //= 4
    for f in (2, 3, 5, 7):
        while r % f == 0:
            rad.append(f)
            r //= f
    f = 11
    while f * f <= r:
        while r % f == 0:
            rad.append(f)
            r //= f
        f += 2
    if r > 1:
        rad.append(r)
    return rad


def stockham(a, radices=None):
    """The mixed-radix Stockham transform as the header of anyfft.hip states it, in float64: stage s with
    Ns = R_1..R_{s-1}, output q of butterfly j = sum_r a[j + r N/R] T[r (k + q Ns) N/(Ns R) mod N],
    k = j mod Ns, written to (j / Ns) Ns R + k + q Ns, T[m] = e^{-2 pi i m / N}. (All N outputs of a stage
    at once, one numpy operation per r.)"""
    a = np.asarray(a, np.complex128).copy()
    N = len(a)
    radices = fft_radices(N) if radices is None else radices
    T = np.exp(-2j * np.pi * np.arange(N) / N)
    it = np.arange(N)
    Ns = 1
    for Rd in radices:
        NR, step = N // Rd, N // (Ns * Rd)
        j, q = it % NR, it // NR
        k = j % Ns
        eq = (k + q * Ns) * step
        acc = np.zeros(N, np.complex128)
        for r in range(Rd):
            acc += a[j + r * NR] * T[(r * eq) % N]
        b = np.empty(N, np.complex128)
        b[(j // Ns) * Ns * Rd + k + q * Ns] = acc
        a = b
        Ns *= Rd
    assert Ns == N
    return a
