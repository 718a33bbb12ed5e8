"""Model of csrc/peaks.hpp: the three pieces of scipy.signal.find_peaks the feature kernels share, in plain
Python, so that tests/test_peaks.py can hold the header to it (and both to scipy where scipy has a rule).

  local_maxima(x)             scipy's _local_maxima_1d: a strict rise, a plateau, a strict fall; the peak is the
                              plateau's middle (left + right) // 2, never the first or last sample
  prominence(x, p)            scipy's _peak_prominences with wlen=None, the difference in float64
  select_by_distance(...)     scipy's _select_by_peak_distance in rounds over flags, as the kernels run it: an
                              undecided peak that no undecided peak within d - 1 beats is kept; an undecided peak
                              that is kept or has a kept peak within d - 1 is decided. Returns the kept peaks
                              and the number of rounds.

Equal heights: the kernels' rule is "the later index wins" (later_wins=True). scipy orders equal priorities by
an unstable argsort and has no such rule, so on ties the header is held to this model alone. later_wins=False
is the opposite rule; the GPU cases use it to show that their expected values depend on the choice."""
import bisect

import numpy as np


def local_maxima(x):
    n, out = len(x), []
    for i in range(1, n - 1):
        if not x[i - 1] < x[i]:
            continue
        j = i + 1
        while j < n - 1 and x[j] == x[i]:
            j += 1
        if x[j] < x[i]:
            out.append((i + j - 1) // 2)
    return out


def prominence(x, p):
    n, h = len(x), x[p]
    lmin = rmin = h
    j = p
    while j >= 0 and x[j] <= h:
        lmin = min(lmin, x[j])
        j -= 1
    j = p
    while j < n and x[j] <= h:
        rmin = min(rmin, x[j])
        j += 1
    return float(np.float64(h) - np.float64(max(lmin, rmin)))


def select_by_distance(x, candidates, d, later_wins=True):
    """candidates: the peak indices, ascending (the header's [lo, hi) is the range that holds them: its
    window clipping only keeps the flag reads inside it). Returns (kept peaks ascending, rounds)."""
    cand = list(candidates)
    near = {i: cand[bisect.bisect_left(cand, i - d + 1):bisect.bisect_right(cand, i + d - 1)] for i in cand}
    und, kept, rounds = set(cand), set(), 0

    def beats(j, i):
        return x[j] > x[i] or (x[j] == x[i] and (j > i if later_wins else j < i))

    while und:
        rounds += 1
        kept |= {i for i in und if not any(j != i and j in und and beats(j, i) for j in near[i])}
        und = {i for i in und if not any(j in kept for j in near[i])}
    return sorted(kept), rounds
