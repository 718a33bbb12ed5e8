"""Plain float64 restatement of MultiResolutionFFT.process_audio_chunk plus combine_results_optimized
(multi_resolution_fft.py:228-302, :335-408) for one frame: the reference of tests/test_combine_plans.py.

It shares no arithmetic with the float32 oracle (oracle/omega_ref.py) beyond the float32 constants the
reference itself holds in float32 -- the window (:177-188), the psychoacoustic weight table (:310-326)
and the resolution weights as the float32 accumulators see them -- and none with the device's combine
plan: every spectrum is a float64 np.fft.rfft and every combine an np.interp over the valid bins.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from oracle import omega_ref as R


def targets(fs: float, max_freq: float, target_bins: int) -> np.ndarray:
    """np.linspace(0, min(max_freq, nyquist), T) (multi_resolution_fft.py:146, :351)."""
    return np.linspace(0, min(max_freq, fs / 2), target_bins)


def magnitudes(x: np.ndarray, configs: Sequence[R.FFTConfig], fs: float,
               apply_weighting: bool = True) -> Dict[int, np.ndarray]:
    """Per resolution |rfft(float64(x[-N:]) * float64(window_f32(N)))|, times float64(psycho_weights)
    when weighting is on (multi_resolution_fft.py:264-279); resolutions longer than x are absent."""
    x = np.asarray(x, np.float32).astype(np.float64)
    out: Dict[int, np.ndarray] = {}
    for i, cfg in enumerate(configs):
        n = cfg.fft_size
        if len(x) < n:
            continue
        mag = np.abs(np.fft.rfft(x[-n:] * R.window_f32(n, cfg.window).astype(np.float64)))
        if apply_weighting:
            mag = mag * R.psycho_weights(cfg, fs).astype(np.float64)
        out[i] = mag
    return out


def combine_given(mags: Dict[int, np.ndarray], configs: Sequence[R.FFTConfig], fs: float, max_freq: float,
                  target_bins: int) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's combine rule in float64 over the GIVEN magnitudes (any subset of the resolutions,
    keyed by resolution index): valid bins in the inclusive range, a resolution with fewer than 2 of them
    skipped (:367-374); targets in the inclusive range (:377-379); np.interp over the valid bins (:383);
    the weighted sum with the float32(weight) values (:387-388); divided wherever the weight sum is above
    0 (:393-395). Returns (combined float64[T], owners int[T])."""
    tgt = targets(fs, max_freq, target_bins)
    acc = np.zeros(target_bins, np.float64)
    wsum = np.zeros(target_bins, np.float64)
    owners = np.zeros(target_bins, np.int64)
    for i in sorted(mags):
        cfg = configs[i]
        mag = np.asarray(mags[i]).astype(np.float64)
        freqs = np.fft.rfftfreq(cfg.fft_size, 1 / fs)
        lo, hi = cfg.freq_range
        valid = (freqs >= lo) & (freqs <= hi)
        if valid.sum() < 2:
            continue
        tmask = (tgt >= lo) & (tgt <= hi)
        if not tmask.any():
            continue
        w = float(np.float32(cfg.weight))
        acc[tmask] += np.interp(tgt[tmask], freqs[valid], mag[valid]) * w
        wsum[tmask] += w
        owners[tmask] += 1
    ok = wsum > 0
    acc[ok] /= wsum[ok]
    return acc, owners


def reference(x: np.ndarray, configs: Sequence[R.FFTConfig], fs: float, max_freq: float, target_bins: int,
              apply_weighting: bool = True) -> Tuple[np.ndarray, np.ndarray, Dict[int, np.ndarray]]:
    """One frame through both steps: (combined float64[T], owners per target int[T], {i: magnitudes})."""
    mags = magnitudes(x, configs, fs, apply_weighting)
    comb, owners = combine_given(mags, configs, fs, max_freq, target_bins)
    return comb, owners, mags


def owned_rms(ref: np.ndarray, owners: Optional[np.ndarray] = None) -> float:
    """Root mean square of the reference over the owned targets (over everything without owners)."""
    v = np.asarray(ref, np.float64)
    if owners is not None:
        v = v[np.asarray(owners) > 0]
    return float(np.sqrt(np.mean(v ** 2)))
