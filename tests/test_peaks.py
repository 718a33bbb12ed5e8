"""The shared find_peaks pieces (csrc/peaks.hpp: local_max_at, prominence, distance_top, distance_decided) on
the CPU: tests/abi/peaks_dump.cpp, a stand-alone host program, evaluates the header on every array below, with
float32 data and byte flags and with float64 data and int flags as the kernels use them, and its peaks,
prominences, kept peaks and round counts must equal tools/model/peaks_model.py's -- and scipy's wherever scipy
has a rule:
  1. every array of length 3..9 over {0, 1, 2} (plateaus of every width and position, also into either end):
     local maxima = model = find_peaks(x); prominences = peak_prominences bit for bit
  2. random permutations (no equal heights), n 3..400, d 1..50: kept peaks = model = find_peaks(x, distance=d)
  3. equal heights: kept peaks = model ("the later index wins"). NOT scipy: it orders equal priorities by an
     unstable argsort and differs from the kernels' rule on some of these arrays (csrc/peaks.hpp).
  4. a staircase of peaks d - 1 apart: one peak is decided per two-peak step, 11 rounds for 22 peaks
and for every array the rounds number at most the candidates (every round decides at least one peak)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import signal

from conftest import REPO
from host_program import compile_host_program

sys.path.insert(0, os.path.join(REPO, "tools", "model"))
import peaks_model as M  # noqa: E402

SRC = os.path.join(REPO, "tests", "abi", "peaks_dump.cpp")
TYPES = (("f", np.float32), ("d", np.float64))
DISTANCES = (1, 2, 3, 10, 20, 50)


def small_arrays():
    return [np.array(v) for n in range(3, 10) for v in itertools.product((0, 1, 2), repeat=n)]


def permutations():
    """(x, d): 3,000 permutations of 0..n-1, every distance 500 times"""
    rng = np.random.default_rng(20240)
    return [(rng.permutation(int(rng.integers(3, 401))), DISTANCES[k % 6]) for k in range(3000)]


def tie_arrays():
    """(x, d, lo, hi): the small arrays at d = 2 and 3, then 600 random arrays over four values, every other
    one over a sub-range [lo, hi) as pitch.hip uses the rule"""
    out = [(x, d, 0, len(x)) for d in (2, 3) for x in small_arrays()]
    rng = np.random.default_rng(20241)
    for k in range(600):
        n = int(rng.integers(20, 401))
        lo, hi = (int(rng.integers(0, n // 3)), int(rng.integers(2 * n // 3, n + 1))) if k & 1 else (0, n)
        out.append((rng.integers(0, 4, n), (2, 3, 10, 20)[(k >> 1) % 4], lo, hi))
    return out


def staircase(d=10, n=200, peaks=22):
    x = np.zeros(n)
    x[5 + (d - 1) * np.arange(peaks)] = 1 + np.arange(peaks)
    return x


def line(t, x, d=1, lo=0, hi=None):
    return " ".join(map(str, [t, len(x), d, lo, len(x) if hi is None else hi] + [int(v) for v in x]))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = compile_host_program(SRC, str(tmp_path_factory.mktemp("peaks") / "peaks_dump"))

    def run(lines):
        """[(peaks, prominences, kept, rounds)] per line"""
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
        out = []
        for ln in r.stdout.splitlines():
            v = ln.split()
            P = int(v[0])
            K = int(v[1 + 2 * P])
            assert len(v) == 3 + 2 * P + K
            out.append(([int(s) for s in v[1:1 + P]], [float(s) for s in v[1 + P:1 + 2 * P]],
                        [int(s) for s in v[2 + 2 * P:2 + 2 * P + K]], int(v[-1])))
        assert len(out) == len(lines)
        return out
    return run


def test_local_maxima_and_prominences_are_scipys_on_every_small_array(dump):
    xs = small_arrays()
    assert len(xs) == 29511
    for t, dtype in TYPES:
        got = dump([line(t, x) for x in xs])
        n_plateau = 0
        for x, (pk, prom, kept, rounds) in zip(xs, got):
            xt = x.astype(dtype)
            want = signal.find_peaks(xt)[0]
            assert pk == list(want) == M.local_maxima(xt), (t, x)
            assert prom == list(signal.peak_prominences(xt, want)[0]) == [M.prominence(xt, p) for p in want], (t, x)
            assert kept == pk and rounds == (1 if pk else 0), (t, x)  # (distance 1 keeps every peak, in one round)
            n_plateau += any(x[p] == x[p + 1] or x[p] == x[p - 1] for p in pk)
        assert n_plateau > 5000  # (peaks that are plateaus, in that many of the arrays)


def test_distance_rule_is_scipys_without_equal_heights(dump):
    cases = permutations()
    assert len(cases) == 3000 and {d for _, d in cases} == set(DISTANCES)
    removed = 0
    for t, dtype in TYPES:
        got = dump([line(t, x, d) for x, d in cases])
        for (x, d), (pk, _, kept, rounds) in zip(cases, got):
            xt = x.astype(dtype)
            want, want_rounds = M.select_by_distance(xt, M.local_maxima(xt), d)
            assert kept == want == list(signal.find_peaks(xt, distance=d)[0]), (t, d, x)
            assert rounds == want_rounds <= len(pk), (t, d, x)
            removed += len(pk) - len(kept)
    assert removed > 50000  # (the rule had work to do)


def test_distance_rule_with_equal_heights_is_the_models(dump):
    """Held to the model alone: "the later index wins" is the kernels' rule, scipy has none (module docstring)."""
    cases = tie_arrays()
    assert len(cases) == 2 * 29511 + 600
    decided_by_tie = 0
    for t, dtype in TYPES:
        got = dump([line(t, x, d, lo, hi) for x, d, lo, hi in cases])
        for (x, d, lo, hi), (pk, _, kept, rounds) in zip(cases, got):
            cand = [p for p in pk if lo <= p < hi]
            want, want_rounds = M.select_by_distance(x, cand, d)
            assert kept == want, (t, d, lo, hi, x)
            assert rounds == want_rounds <= len(cand), (t, d, lo, hi, x)
            decided_by_tie += want != M.select_by_distance(x, cand, d, later_wins=False)[0]
    assert decided_by_tie > 1000  # (arrays on which the opposite tie rule keeps other peaks)


def test_round_structure_on_a_staircase(dump):
    x = staircase()
    for t, dtype in TYPES:
        (pk, _, kept, rounds), = dump([line(t, x, 10)])
        assert len(pk) == 22 and np.all(np.diff(pk) == 9)
        want, want_rounds = M.select_by_distance(x, pk, 10)
        assert kept == want == list(signal.find_peaks(x.astype(dtype), distance=10)[0]) == pk[1::2]
        assert rounds == want_rounds == 11
