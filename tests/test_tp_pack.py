"""The true peak's phase inputs built from the packed forward transform (csrc/rfkern.hip
truepeak_rf_body): the identity restated in float64 numpy (tools/model/tp_pack_model.py) against the
oracle on the CPU, and the register-FFT kernels against the oracle on signals that separate the phases
and the edge bins.

Signals, 8 frames per length (16384 and 8192: the lengths capi_level.cpp / capi_batch.cpp send to
launch_truepeak_rf): DC; the Nyquist alternation +-a (the bin weighted cos(pi p / 4)); a bin-centred
sine; a sine at fs/4 with phase pi/4 (samples +-a/sqrt 2, the peak a between them); impulses at n = 0 and
n = M - 1 (every bin, across the wrap); a sine at 3 fs/8 whose maximum lies on phase 2 alone (phases 1
and 3 reach 0.981 of it, the samples 0.924); seeded noise.

Tolerance: 1e-3 dB against the oracle in float64, the bar of the cfg2 test. The float32 restatement of
the same form (tp_pack_model.phase_peaks_f32) is held to 2 eps32 log2(4N) relative (two float32
transforms in series: 3.3e-5 dB at 16384, thirty times inside the bar) in test_float32_form_has_room;
on these frames it comes within 1e-6 dB of the oracle.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "model"))
import tp_pack_model as P  # noqa: E402
from oracle import omega_ref as R  # noqa: E402

FS = 48000
LENGTHS = [16384, 8192]
TOL_DB = 1e-3
NAMES = ["dc", "nyquist", "bin_sine", "quarter_rate", "impulse_first", "impulse_last", "phase2_sine", "noise"]


def signals(n):
    t = np.arange(n, dtype=np.float64)
    first, last = np.zeros(n), np.zeros(n)
    first[0], last[-1] = 0.8, -0.6
    x = np.stack([
        np.full(n, 0.25),
        0.5 * np.cos(np.pi * t),
        0.5 * np.sin(2 * np.pi * 37 * t / n + 0.3),
        0.6 * np.sin(2 * np.pi * t / 4 + np.pi / 4),
        first,
        last,
        0.5 * np.cos(2 * np.pi * (3 * n // 8) * (t - 0.5) / n),
        0.2 * np.random.default_rng(n).standard_normal(n),
    ])
    return x.astype(np.float32)


_expected = {}


def expected(n):
    """oracle true peak (float64) of the float32 frames, computed once per length"""
    if n not in _expected:
        _expected[n] = np.array([R.true_peak(f.astype(np.float64)) for f in signals(n)])
    return _expected[n]


# ---- CPU: the model ----

@pytest.mark.parametrize("n", LENGTHS + [64])
def test_model_matches_oracle(n):
    """S in both forms, the phase inputs against the unpack / rotate / re-pack form they replace, each
    phase signal against the oracle's resample, and the true peak."""
    rng = np.random.default_rng(1)
    for x in list(signals(n).astype(np.float64)) + [rng.standard_normal(n)]:
        F = P.forward(x)
        S = P.s_term(F)
        scale = max(np.max(np.abs(F)), 1e-300)
        assert np.max(np.abs(S - P.s_term_from_halves(F))) <= 1e-12 * scale
        y4 = R.resample_fft(x, 4 * n)
        for p in (1, 2, 3):
            assert np.max(np.abs(P.phase_input(F, S, p) - P.phase_input_untangled(F, p))) <= 1e-12 * scale
            np.testing.assert_allclose(P.phase_signal(x, p), y4[p::4], rtol=0, atol=1e-12 * np.max(np.abs(y4)))
        assert abs(P.true_peak_db(x) - R.true_peak(x)) <= 1e-10


@pytest.mark.parametrize("n", LENGTHS)
def test_signals_separate_phases_and_edges(n):
    ph = np.array([P.phase_peaks(f) for f in signals(n).astype(np.float64)])
    i = NAMES.index
    assert np.ptp(ph[i("dc")]) < 1e-12
    ny = ph[i("nyquist")]  # a |cos(pi p / 4)|
    assert abs(ny[1] - 0.5 * np.sqrt(0.5)) < 1e-9 and abs(ny[3] - ny[1]) < 1e-9 and ny[2] < 1e-9
    q = ph[i("quarter_rate")]
    assert int(np.argmax(q)) == 2 and abs(q[2] - 0.6) < 1e-6 and abs(q[0] - 0.6 / np.sqrt(2)) < 1e-6
    assert abs(q[1] - q[3]) < 1e-9 and q[1] > q[0] * 1.2
    for nm in ("impulse_first", "impulse_last"):
        a = ph[i(nm)]
        assert int(np.argmax(a)) == 0 and a[1] > 0.85 * a[0] and a[3] > 0.85 * a[0] and a[1] != a[2]
    s = ph[i("phase2_sine")]
    assert int(np.argmax(s)) == 2 and s[2] > 1.015 * max(s[0], s[1], s[3])


@pytest.mark.parametrize("n", LENGTHS)
def test_float32_form_has_room(n):
    """the form in float32 arithmetic against the float64 oracle: far inside the device bar"""
    want = expected(n)
    bar = 20.0 * np.log10(1.0 + 2.0 * float(np.finfo(np.float32).eps) * np.log2(4.0 * n))
    assert bar <= TOL_DB / 30
    for nm, f, w in zip(NAMES, signals(n), want):
        peak = float(np.max(P.phase_peaks_f32(f)))
        err = abs(20.0 * np.log10(peak) - w)
        print(f"n={n} {nm}: float32 form {err:.2e} dB from the oracle")
        assert err <= bar, (n, nm, err)


# ---- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_true_peak_kernel_matches_oracle(n):
    from omega_gpu import Engine, Resolution
    eng = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)
    got = eng.true_peak(signals(n), 4)
    eng.close()
    want = expected(n)
    for nm, g, w in zip(NAMES, got, want):
        print(f"n={n} {nm}: device {float(g):.6f} dB, oracle {w:.6f} dB, diff {abs(float(g) - w):.2e}")
    for nm, g, w in zip(NAMES, got, want):
        assert abs(float(g) - w) <= TOL_DB, (n, nm, float(g), w)


@pytest.mark.gpu
def test_batch_role_matches_oracle_and_standalone_bitwise():
    """omega_process_frames on 4 frames x 2 channels of 16384 (the batch kernel's true-peak role) against the
    oracle, and bitwise against omega_true_peak on the same frames: they share the body."""
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    n = 16384
    x = signals(n)
    e = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    batch = np.asarray(e.process_frames(x.reshape(-1), 4, 2 * n, n)["true_peak_db"])
    alone = e.true_peak(x, 4)
    e.close()
    want = expected(n)
    for nm, g, w in zip(NAMES, batch, want):
        print(f"batch {nm}: device {float(g):.6f} dB, oracle {w:.6f} dB, diff {abs(float(g) - w):.2e}")
    for nm, g, w in zip(NAMES, batch, want):
        assert abs(float(g) - w) <= TOL_DB, (nm, float(g), w)
    np.testing.assert_array_equal(batch, alone)
