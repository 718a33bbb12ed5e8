"""The any-length windowed rfft (anyfft.hip, any_rfft_kernel) bin by bin on designed signals: every radix
schedule of fft_radices the fast kernels do not serve, both sides of the LDS / global-scratch boundary,
more than one scratch slice of run_any, every output selection and window, through Engine.rfft,
GPUAcceleratedFFT and BatchedFFTProcessor, against the float64 expectation of tests/any_rfft_ref.py.

Signals (any_rfft_ref.designed): unit impulses at 0, 1, n//3, n-1 (every bin of magnitude 1 under the
rectangular window: a misplaced output or a wrong twiddle power turns single phases), on-bin tones, the
Nyquist tone, DC, a ramp (not symmetric) and the noise of test_gpu_parity.py's any-length lines.

Tolerance, the rule of tests/test_true_peak_phases.py restated for a spectrum. Per frame and window, `dev`
is the reference's own float32 path (oracle gpu_fft on the float32 frame) against the float64 expectation,
max_k |X32 - X64| / max_k |X64|. A device spectrum may differ from the expectation, in the same measure, by
    bar = max(4 dev, min(FACTOR[path] dev, cap(n))) + eps32 / 2,   cap(n) = eps32 log2(2n)
(4: another transform and summation order; eps32 / 2: half an ulp of the largest bin, for the frames on
which pocketfft happens to be exact), and always by less than SPEC_TOL = 1e-4. A frame whose windowed
product is exactly zero (an impulse under a window's zero end point) must come back exactly zero. The
magnitude output meets the same bar against |X64| and lies within 2 float32 ulps of |.| of the device's
own complex output (sqrtf(re^2 + im^2) of the same registers).

Paths by frame length (run_any): any_lds up to kAnyLdsMax = 6826 points, any_global (scratch) above.
Schedules: SCHEDULES below, pinned on the CPU against any_rfft_ref.fft_radices, whose Stockham restatement
of anyfft.hip's header comment reproduces np.fft.fft on each of them.

Observed on an MI355X (run with -s), over every frame, window and output compared here: worst device
error / worst reference float32 error (both of max |X|) / worst (device error - eps32/2) as a fraction of
cap(n): any_lds 1.82e-7 / 6.5e-8 / 0.10, any_global 3.88e-7 / 1.15e-7 / 0.17 (the magnitude output of
test_scratch_slices; 3.2e-7 / 0.14 on the designed frames, 32768 points with hann). Frames the reference's float32 path gets exactly
(dev = 0) come back within 2.4e-8, under the half ulp. The launch with 163 824 B of dynamic LDS at 6826
points succeeds for both kernels, 6827 runs on scratch, and 171 frames of 32768 points run as slices of
85, 85 and 1. FACTOR was widened to 10 (any_lds) and 6.5 (any_global): the forcing cases stand beside it.

These tests did not change the rfft; tests/test_true_peak_phases.py at the new length 6827 did change the
transform. A stage of a remaining prime R > 7 summed its R terms in float64 but with the float32 twiddle
table, whose rounding errors add up over the terms to one offset common to all outputs: at the prime
6827 every bin k != 0 of a constant frame got 0.25 sum_m (T32[m] - T[m]), and the true peak's inverse
transforms add those up again -- 2.40e-5 dB (4x) and 1.73e-5 dB (2x) off on `dc` against bars of 2.53e-5
and 1.70e-5. Such stages now read an unrounded float64 table (1.4e-7 dB on the same frame).
"""
import numpy as np
import pytest

import any_rfft_ref as A
import true_peak_ref as T
from oracle import omega_ref as R

FS = 48000
EPS32 = float(np.finfo(np.float32).eps)
SPEC_TOL = 1e-4
KANY_LDS_MAX = 6826  # params.hpp kAnyLdsMax: 3 N float2 in 160 KiB of LDS
SCRATCH_FLOAT2 = 8 << 20  # run_any: the scratch of one slice stays within 8 Mi float2

SCHEDULES = {
    1: [], 2: [2], 3: [3], 8: [4, 2], 11: [11], 30: [2, 3, 5], 121: [11, 11], 143: [11, 13],
    256: [4, 4, 4, 4], 441: [3, 3, 7, 7], 1001: [7, 11, 13], 1021: [1021], 1331: [11, 11, 11],
    2310: [2, 3, 5, 7, 11], 4800: [4, 4, 4, 3, 5, 5], 6826: [2, 3413], 6827: [6827],
    7000: [4, 2, 5, 5, 5, 7], 10000: [4, 4, 5, 5, 5, 5], 32768: [4] * 7 + [2],
}
LENGTHS = list(SCHEDULES)
ALL_WINDOWS_AT = (30, 1001, 7000)

# FACTOR x dev, never beyond cap(n). 4 is the rule; the wider ones were forced by frames on which pocketfft's
# float32 spectrum lies well within half an ulp of the largest bin, so that 4 x dev is a fraction of the
# rounding of one float32 result. Measured on an MI355X, (err - eps32/2) / dev:
#   any_lds     9.5  (441, hann, ramp: device 1.37e-7, dev 8.17e-9; cap 1.17e-6)
#   any_global  6.1  (32768, rect, impulse at 5069 x 1.535 (test_scratch_slices frame 137), magnitude output:
#                     device 3.88e-7, dev 5.35e-8; cap 1.91e-6; |.| of its complex output 3.33e-7, 5.1)
FACTOR = {"any_lds": 10.0, "any_global": 6.5}


def path_of(n):
    return "any_lds" if n <= KANY_LDS_MAX else "any_global"


def cap(n):
    """eps32 log2(2n): as far as a widened FACTOR x dev may reach (eps32 at n = 1)."""
    return EPS32 * np.log2(2.0 * max(n, 1))


def bar_of(dev, n, path):
    return max(4.0 * dev, min(FACTOR[path] * dev, cap(n))) + 0.5 * EPS32


def windows_of(n):
    return ("rect", "hann", "hamming", "blackman") if n in ALL_WINDOWS_AT else ("rect", "hann")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


WORST = {}  # path -> [err, dev, (err - eps32/2) / cap] maxima over everything compared so far


def check_bins(label, n, window, names, X64, dev, cp=None, mag=None):
    """Device complex bins `cp` and / or magnitudes `mag` [F, n//2 + 1] against the float64 expectation
    X64 [F, n//2 + 1] with the yardstick dev [F]; returns (worst err, worst dev, worst (err - eps32/2) / cap)."""
    path = path_of(n)
    w = [0.0, 0.0, -np.inf]
    for i, nm in enumerate(names):
        scale = float(np.max(np.abs(X64[i])))
        what = (label, n, window, nm)
        if scale == 0.0:  # x * 0 is exact on both sides
            assert cp is None or not bits(cp[i]).any(), what
            assert mag is None or not bits(mag[i]).any(), what
            continue
        bar = bar_of(dev[i], n, path)
        errs = []
        if cp is not None:
            assert np.isfinite(cp[i]).all(), what
            errs.append(float(np.max(np.abs(cp[i].astype(np.complex128) - X64[i]))) / scale)
        if mag is not None:
            assert np.isfinite(mag[i]).all(), what
            errs.append(float(np.max(np.abs(mag[i].astype(np.float64) - np.abs(X64[i])))) / scale)
        err = max(errs)
        frac = (err - 0.5 * EPS32) / cap(n)
        w = [max(w[0], err), max(w[1], float(dev[i])), max(w[2], frac)]
        print(f"{label} n={n} {window} {nm}: device {err:.2e} of max|X|, reference float32 path {dev[i]:.2e}, "
              f"bar {bar:.2e}, (err - eps32/2)/dev {(err - 0.5 * EPS32) / dev[i] if dev[i] else np.inf:.1f}")
        assert err <= bar and err < SPEC_TOL, what + (errs, float(dev[i]), bar)
    if cp is not None and mag is not None:
        own = np.abs(cp.astype(np.complex128))
        ulp = np.spacing(own.astype(np.float32)).astype(np.float64)
        off = np.abs(mag.astype(np.float64) - own) / ulp
        assert off.max() <= 2.0, (label, n, window, float(off.max()), np.unravel_index(off.argmax(), off.shape))
    acc = WORST.setdefault(path, [0.0, 0.0, -np.inf])
    WORST[path] = [max(a, b) for a, b in zip(acc, w)]
    print(f"{label} n={n} {window} [{path}]: worst device {w[0]:.2e}, worst reference float32 {w[1]:.2e}, "
          f"worst (err - eps32/2)/cap {w[2]:.3f}; {path} so far {WORST[path][0]:.2e} / {WORST[path][1]:.2e} / "
          f"{WORST[path][2]:.3f}")
    return w


# ---- CPU: the signals, the expectation and the documented index map ----

@pytest.mark.parametrize("n", LENGTHS)
def test_closed_forms(n):
    """Impulse (every window), DC, Nyquist and on-bin tone (rect) in closed form against np.fft.rfft of
    the float64 signal times the float32 window, 1e-12 of max |X|; for the signals float32 holds exactly
    that is `expect` of the designed frame itself. Every frame is finite and no two are equal."""
    sig = dict(A.signals64(n))
    seen = 0
    for window in A.WINDOWS:
        names, closed, frames = A.designed(n, window)
        assert list(sig) == names and frames.dtype == np.float32 and frames.shape == (len(names), n)
        assert np.isfinite(frames).all()
        w = A.window64(n, window)
        np.testing.assert_array_equal(w, R.window_f32(n, window).astype(np.float64))
        for i, nm in enumerate(names):
            kind = nm.split("_")[0]
            if closed[nm] is None:
                assert kind in ("ramp", "noise") or window != "rect", (nm, window)
                continue
            seen += 1
            exact = kind in ("impulse", "dc", "nyquist")
            assert not exact or (frames[i].astype(np.float64) == sig[nm]).all()
            X =np.fft.rfft(sig[nm] * w)
            tol = 1e-12 * max(float(np.max(np.abs(closed[nm]))), 1e-300)
            assert np.max(np.abs(X - closed[nm])) <= tol, (nm, window)
            if exact:
                assert np.max(np.abs(A.expect(frames[i], window) - closed[nm])) <= tol, (nm, window)
    assert seen >= 4 * len(A.impulse_positions(n)) + len(A.tone_bins(n)) + 1 + (n % 2 == 0)
    if n > 3:  # (at 1-3 points a tone, DC and an impulse can coincide)
        _, _, frames = A.designed(n, "rect")
        assert len({f.tobytes() for f in frames}) == len(frames)
    X64, dev = A.reference(n, "hann")
    assert X64.shape == (len(frames), n // 2 + 1) and (dev < SPEC_TOL / 4).all()


@pytest.mark.parametrize("n", LENGTHS)
def test_stage_recurrence(n):
    """The schedule of fft_radices and the stage recurrence of anyfft.hip's header comment (inputs
    a[j + r N/R], twiddle index r (k + q Ns) N/(Ns R) mod N, output slot (j/Ns) Ns R + k + q Ns), restated
    in float64, give np.fft.fft on a random complex vector to 1e-10 of max |X|."""
    rad = A.fft_radices(n)
    assert rad == SCHEDULES[n] and int(np.prod(rad, dtype=np.int64)) == n
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    want = np.fft.fft(a)
    got = A.stockham(a, rad)
    assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))


def test_tolerance_rule():
    assert cap(1) == EPS32 and abs(cap(4800) - EPS32 * np.log2(9600)) < 1e-20
    for path in FACTOR:
        assert FACTOR[path] >= 4.0
        assert bar_of(0.0, 1000, path) == 0.5 * EPS32
        assert bar_of(1e-3, 1000, path) == 4e-3 + 0.5 * EPS32  # beyond cap: 4 dev alone
    assert path_of(KANY_LDS_MAX) == "any_lds" and path_of(KANY_LDS_MAX + 1) == "any_global"
    assert 3 * KANY_LDS_MAX * 8 <= 160 * 1024 - 16 < 3 * (KANY_LDS_MAX + 1) * 8


# ---- GPU ----

@pytest.fixture(scope="module")
def eng():
    from omega_gpu import Engine, Resolution
    return Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_bins_designed(eng, n):
    """Engine.rfft with both outputs over all designed frames of one length in one call, rect and hann
    (all four windows at 30, 1001, 7000): every bin of the complex and the magnitude output."""
    for window in windows_of(n):
        names, _, frames = A.designed(n, window)
        X64, dev = A.reference(n, window)
        mag, cp = eng.rfft(frames, window, magnitude=True, complex_out=True)
        assert mag.shape == cp.shape == X64.shape
        check_bins("rfft", n, window, names, X64, dev, cp, mag)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [30, KANY_LDS_MAX, 7000])
def test_output_selection(eng, n):
    """`mag` only and `cplx` only return bitwise the arrays of the both-outputs call, and a second
    identical call is bitwise equal."""
    for window in ("rect", "hann"):
        _, _, frames = A.designed(n, window)
        mag, cp = eng.rfft(frames, window, magnitude=True, complex_out=True)
        m_only, none_c = eng.rfft(frames, window, magnitude=True, complex_out=False)
        none_m, c_only = eng.rfft(frames, window, magnitude=False, complex_out=True)
        assert none_c is None and none_m is None
        np.testing.assert_array_equal(bits(m_only), bits(mag), err_msg=f"n={n} {window} mag only")
        np.testing.assert_array_equal(bits(c_only), bits(cp), err_msg=f"n={n} {window} cplx only")
        mag2, cp2 = eng.rfft(frames, window, magnitude=True, complex_out=True)
        np.testing.assert_array_equal(bits(mag2), bits(mag), err_msg=f"n={n} {window} second call")
        np.testing.assert_array_equal(bits(cp2), bits(cp), err_msg=f"n={n} {window} second call")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1001, KANY_LDS_MAX, KANY_LDS_MAX + 1, 10000])
def test_frames_are_independent(eng, n):
    """Each row of a batch of 9 different frames is bitwise that frame transformed alone (on the scratch
    path: no two workgroups share or overlap their 3N scratch rows)."""
    for window in ("rect", "hann"):
        _, _, frames = A.designed(n, window)
        frames = frames[-9:]
        assert len(frames) == 9 and len({f.tobytes() for f in frames}) == 9
        mag, cp = eng.rfft(frames, window)
        for i, f in enumerate(frames):
            m1, c1 = eng.rfft(f, window)
            np.testing.assert_array_equal(bits(m1[0]), bits(mag[i]), err_msg=f"n={n} {window} frame {i} mag")
            np.testing.assert_array_equal(bits(c1[0]), bits(cp[i]), err_msg=f"n={n} {window} frame {i} cplx")


@pytest.mark.gpu
def test_scratch_slices(eng):
    """32768 points, 171 frames: two full scratch slices of run_any and a one-frame slice. Frame f is an
    impulse at 37 f mod N scaled by 1 + f/256, so every frame has its own phase ramp and level. Bins on
    the frames around the slice boundaries, |X| on every bin of every frame; host memory with rect through
    Engine.rfft, device memory with hann (complex only) through GPUAcceleratedFFT.process_fft_batch."""
    import torch
    from omega_gpu.gpu_accelerated_fft import GPUAcceleratedFFT
    n, F = 32768, 171
    per = SCRATCH_FLOAT2 // (3 * n)
    assert n > KANY_LDS_MAX and per == 85 and F > 2 * per and F == 2 * per + 1
    edge = [0, per - 1, per, per + 1, 2 * per - 1, 2 * per]
    x = np.zeros((F, n), np.float32)
    pos = [(37 * f) % n for f in range(F)]
    for f in range(F):
        x[f, pos[f]] = np.float32(1.0 + f / 256.0)
    assert len(set(pos)) == F
    names = [f"frame_{f}" for f in range(F)]
    ga = GPUAcceleratedFFT()
    for window in ("rect", "hann"):
        X64 = np.stack([A.expect(r, window) for r in x])
        dev = np.array([0.0 if not X.any() else A.deviation(A.yardstick(r, window), X) for r, X in zip(x, X64)])
        level = np.array([x[f, pos[f]] * A.window64(n, window)[pos[f]] for f in range(F)], np.float64)
        np.testing.assert_allclose(np.abs(X64), np.broadcast_to(np.abs(level)[:, None], X64.shape), rtol=1e-12, atol=0)
        if window == "rect":
            mag, cp = eng.rfft(x, window, magnitude=True, complex_out=True)
            check_bins("slices host mag", n, window, names, X64, dev, None, mag)
        else:
            assert level[0] == 0.0 and (level[1:] > 0).all()  # (the hann window's zero end point)
            out = ga.process_fft_batch(torch.from_numpy(x).cuda(), window)
            assert out is not None and out.is_cuda and out.dtype == torch.complex64 and out.shape == (F, n // 2 + 1)
            cp = out.cpu().numpy()
        # |X| of every frame is the frame's level at every bin
        check_bins("slices |X|", n, window, names, np.abs(X64), dev, None, np.abs(cp.astype(np.complex128)))
        check_bins("slices bins", n, window, [names[f] for f in edge], X64[edge], dev[edge], cp[edge],
                   mag[edge] if window == "rect" else None)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [KANY_LDS_MAX, KANY_LDS_MAX + 1])
def test_lds_boundary(eng, n):
    """The largest length in LDS (3 N float2 = 163 824 B of dynamic LDS, with the true-peak kernel's 16 B
    of static LDS exactly 160 KiB) and the first one on global scratch: the rfft and the 4x true peak both
    launch and are right."""
    import test_true_peak_phases as TP
    assert TP.path_of(n) == path_of(n) == ("any_lds" if n == KANY_LDS_MAX else "any_global")
    for window in ("rect", "hann"):
        names, _, frames = A.designed(n, window)
        X64, dev = A.reference(n, window)
        mag, cp = eng.rfft(frames, window, magnitude=True, complex_out=True)
        check_bins("boundary rfft", n, window, names, X64, dev, cp, mag)
    names, _, frames = T.designed(n)
    got = eng.true_peak(frames, 4)
    TP.check_values("boundary true peak", path_of(n), n, got, names, frames, T.reference(n), 4)


@pytest.mark.gpu
def test_facade_routing():
    """BatchedFFTProcessor groups a padded 1000-point rect request and a trimmed 7000-point hamming request
    of one process_batch onto the any-length kernel (LDS and scratch); GPUAcceleratedFFT.compute_fft at one
    and two points."""
    from omega_gpu.batched_fft_processor import BatchedFFTProcessor
    from omega_gpu.gpu_accelerated_fft import GPUAcceleratedFFT
    from oracle import signals as S
    bp = BatchedFFTProcessor()
    cases = (("pad", S.noise(6, 900, 0.2), 1000, "rect"), ("trim", S.noise(7, 8000, 0.2), 7000, "hamming"))
    ids = {name: bp.prepare_batch(name, x, n, w) for name, x, n, w in cases}
    assert bp.process_batch() == 2
    res = bp.distribute_results()
    for name, x, n, w in cases:
        want = R.batched_fft(x.astype(np.float64), n, w)
        ref32 = R.batched_fft(x, n, w)
        assert want["complex"].dtype == np.complex128 and ref32["complex"].dtype == np.complex64
        got = res[ids[name]]
        assert got["complex"].dtype == np.complex64 and got["magnitude"].dtype == np.float32
        np.testing.assert_array_equal(got["frequencies"], want["frequencies"])
        dev = np.array([A.deviation(ref32["complex"], want["complex"])])
        check_bins("BatchedFFTProcessor", n, w, [name], want["complex"][None], dev, got["complex"][None],
                   got["magnitude"][None])
    for n in (1, 2):
        for window in ("hann", "hamming"):
            x = np.array([0.75, -0.5], np.float32)[:n]
            X64 = A.expect(x, window)
            dev = np.array([0.0 if not X64.any() else A.deviation(A.yardstick(x, window), X64)])
            mag, cp = GPUAcceleratedFFT().compute_fft(x, window)
            assert mag.shape == cp.shape == (n // 2 + 1,) == X64.shape
            check_bins("compute_fft", n, window, [f"tiny_{n}"], X64[None], dev, cp[None], mag[None])
