#!/usr/bin/env python3
"""Model of the true peak's phase inputs built straight from the packed forward transform
(csrc/rfkern.hip truepeak_rf_body): the identity, its edge bins and its scale, in numpy, pinned to
the oracle's true peak (tests/test_tp_pack_model.py).

A frame x of M = 2K samples is packed as z[n] = x[2n] + i x[2n+1], F = FFT_K(z). With E, O the
half-spectra of the even and odd samples (F_k = E_k + i O_k), w = e^{-2 pi i / M} and
X_k = E_k + w^k O_k the real spectrum, phase p of the 4x oversampled signal is
y_p[n] = irfft_M(X_k r^k), r = e^{2 pi i p / 4M} (the Nyquist bin X_K weighted cos(pi p / 4)), and
its packed form y_p[2n] + i y_p[2n+1] is conj(FFT_K(Z')) / K with

  2 conj(Z'_k) = (Y_k + Y') + g_k (Y_k - Y'),  Y_k = X_k r^k,  Y' = conj(Y_{K-k}),  g_k = i w^{-k}.

From conj(X_{K-k}) = E_k - w^k O_k and conj(r)^{K-k} = phi r^k, phi = e^{-i pi p / 4}:

  Y_k + Y' = r^k [(1 + phi) E_k + (1 - phi) w^k O_k]
  Y_k - Y' = r^k [(1 - phi) E_k + (1 + phi) w^k O_k]
  2 conj(Z'_k) = r^k [(1 + phi) (E_k + i O_k) + (1 - phi) (i w^{-k} E_k + w^k O_k)]
               = 2 e^{-i th} r^k [cos(th) F_k + i sin(th) S_k],   th = pi p / 8,

with the phase-independent S_k = i w^{-k} E_k + w^k O_k. Substituting E = (F_k + conj F_{K-k}) / 2 and
O = (F_k - conj F_{K-k}) / 2i collapses S to two real-scaled terms:

  S_k = Im(w^k) F_k + Re(w^k) i conj(F_{K-k}).

k = 0 (F_K read as F_0; S_0 = Im F_0 + i Re F_0): X_0 = Re F_0 + Im F_0 is its own mirror and the
Nyquist bin X_K = Re F_0 - Im F_0 enters with the real weight c = cos(pi p / 4) in place of phi, so

  conj(Z'_0) = cos^2(th) F_0 + sin^2(th) S_0            (1 + c = 2 cos^2 th, 1 - c = 2 sin^2 th).

k = K/2 is its own mirror and follows the general form. The kernel drops the common factor 2 (it
transforms Z', not 2 Z'), applies the thread-common part of r^k after pass 1's DFT16 (it commutes with
it) and takes max |.| / K of the transform's real and imaginary parts.
"""
import numpy as np


def forward(x):
    """F = FFT_K of the even/odd-packed frame"""
    x = np.asarray(x)
    return np.fft.fft(x[0::2] + 1j * x[1::2])


def s_term(F):
    """S_k = Im(w^k) F_k + Re(w^k) i conj(F_{K-k}), k < K (F_K = F_0)"""
    K = len(F)
    k = np.arange(K)
    wk = np.exp(-2j * np.pi * k / (2 * K))
    Fm = np.conj(F[(K - k) % K])
    return wk.imag * F + wk.real * 1j * Fm


def s_term_from_halves(F):
    """S_k = i w^{-k} E_k + w^k O_k from the untangled half-spectra (the definition)"""
    K = len(F)
    k = np.arange(K)
    wk = np.exp(-2j * np.pi * k / (2 * K))
    Fm = np.conj(F[(K - k) % K])
    E, O = (F + Fm) / 2, (F - Fm) / 2j
    return 1j * np.conj(wk) * E + wk * O


def phase_input(F, S, p):
    """conj(Z'_k) of phase p, k < K"""
    K = len(F)
    th = np.pi * p / 8
    k = np.arange(K)
    G = np.exp(-1j * th) * np.exp(2j * np.pi * k * p / (8 * K)) * (np.cos(th) * F + 1j * np.sin(th) * S)
    G[0] = np.cos(th) ** 2 * F[0] + np.sin(th) ** 2 * S[0]
    return G


def phase_input_untangled(F, p):
    """the same from the real spectrum: the form the identity replaces (unpack, rotate, re-pack)"""
    K = len(F)
    k = np.arange(K)
    wk = np.exp(-2j * np.pi * k / (2 * K))
    Fm = np.conj(F[(K - k) % K])
    E, O = (F + Fm) / 2, (F - Fm) / 2j
    X = E + wk * O
    X[0] = F[0].real + F[0].imag
    XK = F[0].real - F[0].imag
    Y = X * np.exp(2j * np.pi * k * p / (8 * K))
    Yp = np.conj(Y[(K - k) % K])
    Yp[0] = XK * np.cos(np.pi * p / 4)
    g = 1j * np.conj(wk)
    return ((Y + Yp) + g * (Y - Yp)) / 2


def phase_signal(x, p):
    """y[4n + p], n < M, of the 4x resampled frame"""
    F = forward(x)
    K = len(F)
    Y = np.fft.fft(np.conj(phase_input(F, s_term(F), p))) / K
    y = np.empty(2 * K)
    y[0::2], y[1::2] = Y.real, -Y.imag  # FFT(Z') = conj(K y packed)
    return y


def phase_peaks(x):
    """max |.| of the four phases (phase 0: the samples)"""
    x = np.asarray(x, np.float64)
    return np.array([np.max(np.abs(x))] + [np.max(np.abs(phase_signal(x, p))) for p in (1, 2, 3)])


def true_peak_db(x):
    peak = float(np.max(phase_peaks(x)))
    return -100.0 if peak < 1e-10 else 20.0 * np.log10(peak)


def phase_peaks_f32(x):
    """the same in float32 arithmetic (complex64 transforms, float32 coefficients): the size of the
    rounding a float32 kernel of this form carries"""
    x = np.asarray(x, np.float32)
    z = (x[0::2] + 1j * x[1::2]).astype(np.complex64)
    F = np.fft.fft(z).astype(np.complex64)
    K = len(F)
    k = np.arange(K)
    wk = np.exp(-2j * np.pi * k / (2 * K)).astype(np.complex64)
    Fm = np.conj(F[(K - k) % K])
    S = (wk.imag * F + wk.real * (1j * Fm).astype(np.complex64)).astype(np.complex64)
    out = [np.float32(np.max(np.abs(x)))]
    for p in (1, 2, 3):
        th = np.pi * p / 8
        rot = (np.exp(-1j * th) * np.exp(2j * np.pi * k * p / (8 * K))).astype(np.complex64)
        H = (np.float32(np.cos(th)) * F + (np.float32(np.sin(th)) * (1j * S)).astype(np.complex64)).astype(np.complex64)
        G = (rot * H).astype(np.complex64)
        G[0] = np.float32(np.cos(th) ** 2) * F[0] + np.float32(np.sin(th) ** 2) * S[0]
        Y = np.fft.fft(np.conj(G)).astype(np.complex64)
        out.append(np.float32(max(np.max(np.abs(Y.real)), np.max(np.abs(Y.imag)))) / np.float32(K))
    return np.array(out, np.float32)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
    from oracle import omega_ref as R
    rng = np.random.default_rng(0)
    for M in (8192, 16384):
        x = 0.25 * np.sin(2 * np.pi * 440 * np.arange(M) / 48000) + 0.05 * rng.standard_normal(M)
        F = forward(x)
        print(M, "S forms", np.max(np.abs(s_term(F) - s_term_from_halves(F))),
              "pack", max(np.max(np.abs(phase_input(F, s_term(F), p) - phase_input_untangled(F, p))) for p in (1, 2, 3)),
              "model", true_peak_db(x), "oracle", R.true_peak(x))
