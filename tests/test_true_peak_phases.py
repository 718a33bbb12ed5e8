"""The 4x true peak, phase by phase, on designed signals: every kernel path of omega_true_peak_os, the
batch launch's true-peak role and omega_calculate_lufs against the float64 restatement
tests/true_peak_ref.py, which is pinned to oracle.omega_ref.resample_fft / true_peak on the CPU.

Signals (true_peak_ref.designed(n), float64 cast to float32): tones at N/4 and band-limited fractional
pulses whose 4x maximum lies on one chosen interpolated phase, 0.69-0.91 dB above the next (the pulses
also across the circular wrap); the Nyquist tone alone and mixed into phase-1 / phase-3 winners, where
its weight cos(pi/4) moves the 4x value by 0.36-0.65 dB; DC, an impulse pair at the frame ends, and frames
0.9x / 1.1x the 1e-10 silence threshold whose peak lies on phase 2 (so 1x stays silent). With the three
oversampling factors (phase 0 / phases 0, 2 / all four) each of phases 1, 2, 3 is identified separately.

Tolerance. Per signal and factor, `dev` is the reference's own float32 path (resample_fft on the float32
frame) against the float64 evaluation of the same frame, in dB. A device value may differ from the
float64 expectation by FACTOR[path] x dev (4: another transform and summation order, as tests/test_pitch.py
and tests/test_harmonic.py) plus half an ulp of the float32 dB value. A factor may be widened for a path
only as far as FACTOR x dev <= eps32 log2(4N) relative (cap_db), with the measurement that forced it
recorded here. The sentinel frames return exactly -100.0 or a finite value on the reference's side.

Paths by frame length (omega_true_peak_os / tp_launch / run_any): 512-4096 launch_truepeak (Stockham),
8192 and 16384 launch_truepeak_rf (register FFT), 1-7, 16, 100, 1000, 1021, 4800, 6826 anyfft.hip in LDS
(radix-4, radix-2/5, a prime single stage; 6826 = 2 x 3413 fills the 160 KiB), 6827 (prime) and 10000
anyfft.hip on global scratch; the batch kernel's
true-peak role and the captured-graph layout at 16384 through process_frames; omega_calculate_lufs at
2048 and 4800.

Observed on an MI355X, max over signals and factors of |device - float64| in dB (run with -s), and the
largest (deviation - half ulp) as a fraction of cap_db(n): any_lds 3.7e-6 dB (0.11, n = 100), any_global
3.5e-6 (0.06), stockham 6.1e-6 (0.47, n = 1024, pulse_wrapN_p1 at 4x; 0.22 elsewhere), rf 3.7e-6 (0.15),
batch and graph as rf at 16384. The 3.x e-6 figures are the above-silence frames, where the device returns
the float32 nearest the expectation at -199.17 dB (half an ulp there is 7.6e-6); on the -6 dB signals the
deviations are 2e-7 to 2.3e-6. Before this module the prime length 1021 summed its single 1021-term
stage in float32 and was 6.5e-5 dB (5.9e-6 relative, 4.6 x cap) off on the above-silence pulse, and
20.0f * log10f(peak) was up to an ulp of the dB value off for an exact peak (DC: 8.1e-7 dB against half an
ulp of 4.8e-7); anyfft.hip now sums radices above 7 in float64 and the three kernels share tp_db(). At 6827 those sums
still took the float32 twiddle table and `dc` was 2.40e-5 dB (4x) / 1.73e-5 dB (2x, bar 1.70e-5) off, the
table's rounding errors adding up to one offset in every bin; with the float64 table 1.4e-7 dB, and
6826 / 6827 3.3e-6 / 3.6e-6 dB at worst (the above-silence frames again).
"""
import ctypes as C

import numpy as np
import pytest

import true_peak_ref as T
from oracle import omega_ref as R

FS = 48000
EPS32 = float(np.finfo(np.float32).eps)
LENGTHS = [1, 2, 3, 5, 7, 16, 100, 512, 1000, 1021, 1024, 2048, 4096, 4800, 6826, 6827, 8192, 10000,
           16384]
FACTORS = (4, 2, 1)


def path_of(n):
    if n in (8192, 16384):
        return "rf"
    if n in (512, 1024, 2048, 4096):
        return "stockham"
    return "any_lds" if n <= 6826 else "any_global"  # kAnyLdsMax


# FACTOR x dev, never beyond cap_db(n). 4 is the rule; the wider ones were forced by signals on which
# pocketfft's float32 maximum lands within a few 1e-9 dB of the float64 one by chance, so that 4 x dev is
# far below one float32 ulp of the peak (1.0e-6 dB). Measured on an MI355X, (err - half ulp) / dev:
#   stockham    2095  (1024, 4x, pulse_wrapN_p1: device 6.13e-6 dB, dev 2.8e-9 dB; cap 1.24e-5 dB)
#   rf          70.8  (8192, 4x, pulse_mid_p3: device 1.81e-6 dB, dev 2.2e-8 dB; cap 1.55e-5 dB)
#   any_lds     18.1  (1000, 2x, pulse_wrapN_p1: device 7.25e-7 dB, dev 2.7e-8 dB; cap 1.24e-5 dB)
#   any_global   6.3  (10000, 4x, tone_p2: device 1.17e-6 dB, dev 1.5e-7 dB; cap 1.58e-5 dB)
# batch and graph run the register-FFT true-peak body at 16384 (43.7 there: nyqmix_pulse_p3).
FACTOR = {"stockham": 2100.0, "rf": 72.0, "any_lds": 19.0, "any_global": 7.0, "batch": 72.0, "graph": 72.0}


def cap_db(n):
    """eps32 log2(4N) relative, in dB: as far as a widened FACTOR x dev may reach."""
    return 20.0 * np.log10(1.0 + EPS32 * np.log2(4.0 * max(n, 1)))


def yardstick(frame, phases, o):
    """|dB of the reference's float32 path - dB of the float64 evaluation| for one frame and factor.
    Where several phases tie for the maximum to within float32 precision (phases 0 and 2 mirror each
    other on the phase-1 / phase-3 signals), any of them may hold a float32 maximum: the largest of their
    deviations counts, not only that of the phase pocketfft's rounding happened to pick (0 when that is
    the samples themselves)."""
    n = len(frame)
    y = R.resample_fft(frame, o * n)
    assert y.dtype == np.float32
    p64 = np.asarray(phases)[:: 4 // o]
    p32 = np.array([float(np.max(np.abs(y[j::o]))) for j in range(o)])
    tied = p64 >= p64.max() * (1.0 - EPS32 * np.log2(4.0 * n))
    return float(np.max(np.abs(20.0 * np.log10(p32[tied] / p64[tied]))))


def check_values(label, path, n, got, names, frames, phases, o):
    """Device values `got` [F] of the designed frames against the float64 expectation; returns the
    largest deviation of the finite ones."""
    worst = 0.0
    for i, nm in enumerate(names):
        want = T.db(T.peak_of(phases[i], o))
        if want == -100.0:
            assert got[i] == -100.0, (label, n, nm, o, got[i])
            continue
        assert np.isfinite(got[i]) and got[i] != -100.0, (label, n, nm, o, got[i])
        dev = yardstick(frames[i], phases[i], o)
        bar = max(4.0 * dev, min(FACTOR[path] * dev, cap_db(n))) + 0.5 * float(np.spacing(np.float32(abs(want))))
        err = abs(float(got[i]) - want)
        worst = max(worst, err)
        print(f"{label} n={n} {o}x {nm}: device {err:.2e} dB from float64, reference float32 path {dev:.2e}, "
              f"bar {bar:.2e}")
        assert err <= bar, (label, n, nm, o, float(got[i]), want, err, bar)
    print(f"{label} n={n} {o}x: worst device deviation {worst:.2e} dB")
    return worst


# ---- CPU: the reference and the signals ----

@pytest.mark.parametrize("n", LENGTHS)
def test_reference_matches_oracle(n):
    """true_peak_ref.phase_peaks is the oracle's resample in float64: identical to 1e-12 for the three
    factors, and through true_peak's threshold."""
    names, _, frames = T.designed(n)
    ph = T.reference(n)
    rng = np.random.default_rng(n)
    extra = rng.standard_normal(n).astype(np.float32)
    for fr, p in list(zip(frames, ph)) + [(extra, T.phase_peaks(extra))]:
        x = fr.astype(np.float64)
        y4 = R.resample_fft(x, 4 * n)
        np.testing.assert_allclose(T.resample4(x), y4, rtol=0, atol=1e-12 * max(np.max(np.abs(y4)), 1e-300))
        for o in FACTORS:
            want = np.max(np.abs(R.resample_fft(x, o * n)))
            assert abs(T.peak_of(p, o) - want) <= 1e-12 * want
            assert abs(T.db(T.peak_of(p, o)) - R.true_peak(x, o)) <= 1e-12 * abs(R.true_peak(x, o))


@pytest.mark.parametrize("n", LENGTHS)
def test_designed_signal_properties(n):
    """Every property the device comparison relies on, on the float64 reference of the float32 frames."""
    names, meta, frames = T.designed(n)
    ph = T.reference(n)
    tp = {nm: [T.db(T.peak_of(ph[i], o)) for o in (1, 2, 4)] for i, nm in enumerate(names)}
    kinds = {k for k, _ in meta.values()}
    assert {"dc", "edge", "sentinel"} <= kinds
    if n >= 16:
        assert "pulse" in kinds and (n % 4 or "tone" in kinds) and (n % 2 or "nyqmix" in kinds)
    for i, nm in enumerate(names):
        kind, p = meta[nm]
        srt = np.sort(ph[i])[::-1]
        gap = 20 * np.log10(srt[0] / srt[1])
        t1, t2, t4 = tp[nm]
        if kind in ("tone", "pulse"):
            assert int(np.argmax(ph[i])) == p, (nm, ph[i])
            assert gap >= (0.6876 if kind == "tone" else 0.91 if n >= 1000 else 0.79), (nm, gap)  # 0.6877 = -dB cos(pi/8)
            assert abs(t4 + 6.0206) < 1e-4
            if p == 2:
                assert t2 == t4 and t1 < t4 - 3.0
            else:
                assert abs(t1 - t2) < 1e-6 and t2 <= t4 - 0.6876  # phases 0 and 2 mirror each other
            if kind == "tone":
                assert abs(t1 - (-9.0309 if p == 2 else -6.7083)) < 1e-4
        elif kind == "nyquist":
            assert (ph[i] <= ph[i][0]).all()
            assert all(abs(t + 6.0206) < 1e-6 for t in (t1, t2, t4))
        elif kind == "nyqmix":
            assert int(np.argmax(ph[i])) == p and p in (1, 3) and gap >= 0.3, (nm, ph[i])
            up = T.expected_db(frames[i], 4, 1.0) - t4
            down = T.expected_db(frames[i], 4, 0.0) - t4
            assert up >= 0.1 and down <= -0.1, (nm, up, down)
            # the weight matters on the interpolated phases only
            assert T.expected_db(frames[i], 1, 1.0) == t1
        elif kind == "dc":
            assert np.ptp(ph[i]) <= 1e-15 and all(abs(t + 12.0412) < 1e-4 for t in (t1, t2, t4))
        elif kind == "edge":
            if n > 1:
                assert frames[i][0] == np.float32(0.7) and frames[i][-1] == np.float32(-0.7)
            assert abs(t1 - 20 * np.log10(float(np.float32(0.7)))) < 1e-9
            if n >= 3:
                assert t4 > t1 + 0.5  # the maximum lies between the two end samples, across the wrap
        elif kind == "sentinel":
            below = nm == "below_silence"
            for o in FACTORS:
                p64 = T.peak_of(ph[i], o)
                p32 = float(np.max(np.abs(R.resample_fft(frames[i], o * n))))
                assert abs(p64 / 1e-10 - 1) > 0.05 and abs(p32 / 1e-10 - 1) > 0.05, (nm, o, p64, p32)
                assert (p64 < 1e-10) == (p32 < 1e-10)  # float32 and float64 references agree on the side
            assert abs(T.peak_of(ph[i], 4) / 1e-10 - (0.9 if below else 1.1)) < 1e-3
            if below:
                assert t1 == t2 == t4 == -100.0
            else:
                assert abs(t4 - 20 * np.log10(1.1e-10)) < 1e-2 and t2 == t4
            if n >= 3:
                assert t1 == -100.0  # phase 0 stays below the threshold either way
    # neighbouring frames of the stacked call differ in their winning phase or level
    for a, b in zip(names, names[1:]):
        assert tp[a] != tp[b] or meta[a][1] != meta[b][1], (a, b)


# ---- GPU ----

@pytest.fixture(scope="module")
def eng():
    from omega_gpu import Engine, Resolution
    return Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_true_peak_os_every_path(eng, n):
    """Engine.true_peak at 4x, 2x and 1x over all designed frames of one length in one call: each value
    against the float64 reference, and the stacked call bitwise equal to one call per frame."""
    names, _, frames = T.designed(n)
    ph = T.reference(n)
    for o in FACTORS:
        got = eng.true_peak(frames, o)
        check_values(path_of(n), path_of(n), n, got, names, frames, ph, o)
        single = np.array([eng.true_peak(f, o)[0] for f in frames], np.float32)
        np.testing.assert_array_equal(got, single, err_msg=f"n={n} {o}x stacked vs one frame per call")


@pytest.mark.gpu
@pytest.mark.parametrize("layout,flags", [("batch", 0), ("graph", 1)])
def test_batch_launch_true_peak(layout, flags):
    """process_frames(meters=True) on the north-star resolutions, 2 channels x 12 frames of 16384 with
    different designed signals on the two channels of a frame: the batch kernel's true-peak role (default
    layout) and the captured-graph layout (first call and replay), each against the float64 reference."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    from omega_gpu import _lib as L
    n, F = 16384, 12
    names, _, frames = T.designed(n)
    ph = T.reference(n)
    idx = [i % len(names) for i in range(2 * F)]
    x = torch.from_numpy(np.ascontiguousarray(frames[idx]).reshape(F, 2, n)).cuda()
    e = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    e._check(L.lib().omega_set_graphs(e._ctx, flags))
    bufs = {k: torch.empty(2 * F, *s, dtype=d, device="cuda") for k, s, d in
            (("combined", (512,), torch.float32), ("lufs_inst", (), torch.float32),
             ("true_peak_db", (), torch.float32), ("meters", (5,), torch.float64))}
    for call in range(2):
        o = e.process_frames(x, F, 2 * n, n, meters=True, out=bufs)
        torch.cuda.synchronize()
        got = o["true_peak_db"].cpu().numpy()
        check_values(f"{layout}[call {call}]", layout, n, got, [names[i] for i in idx], frames[idx], ph[idx], 4)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [2048, 4800])
def test_calculate_lufs_true_peak(n, dtype):
    """omega_calculate_lufs (the true peak on the side stream beside the weighting) through
    Engine.calculate_lufs and the ProfessionalMetering facade, float32 and float64 frames (cast on load)."""
    from omega_gpu import Engine, Resolution
    from omega_gpu.professional_meters import ProfessionalMetering
    names, _, frames = T.designed(n)
    ph = T.reference(n)
    x = frames.astype(dtype)
    e = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512, n_channels=1)
    path = path_of(n)
    for o in FACTORS:
        _, tp, _ = e.calculate_lufs(x, "K", o)
        check_values(f"calculate_lufs[{np.dtype(dtype).name}]", path, n, tp, names, frames, ph, o)
    e.close()
    pm = ProfessionalMetering(FS)
    got = []
    for f in x:
        pm.reset()  # the dict's true_peak is the peak hold of the stream: one frame per stream
        got.append(pm.calculate_lufs(f)["true_peak"])
    check_values(f"facade calculate_lufs[{np.dtype(dtype).name}]", path, n, np.array(got, np.float64), names, frames,
                 ph, 4)
    for o in FACTORS:
        direct = np.array([pm.calculate_true_peak(f, o) for f in x], np.float64)
        check_values(f"facade calculate_true_peak[{np.dtype(dtype).name}]", path, n, direct, names, frames, ph, o)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096, 1000])
def test_device_memory_input_bitwise(n):
    """omega_true_peak_os on device memory (no staging) equals the host-memory call bitwise, one
    power-of-two and one any-length case."""
    import torch
    from omega_gpu import Engine, Resolution
    from omega_gpu import _lib as L
    eng = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)
    names, _, frames = T.designed(n)
    ph = T.reference(n)
    xd = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    for o in FACTORS:
        host = eng.true_peak(frames, o)
        out = torch.full((len(names),), float("nan"), dtype=torch.float32, device="cuda")
        eng._bind_stream(xd)
        eng._check(L.lib().omega_true_peak_os(eng._ctx, C.c_void_p(xd.data_ptr()), len(names), n, o,
                                              C.c_void_p(out.data_ptr()), L.MEM_DEVICE))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), host, err_msg=f"n={n} {o}x")
        check_values("device-memory", path_of(n), n, out.cpu().numpy(), names, frames, ph, o)
