"""Every device path of the windowed power-of-two rfft, bin by bin on designed signals, against the float64
expectation of tests/any_rfft_ref.py (the rule of tests/test_any_rfft.py, unchanged).

Paths (PATHS), how each is reached, and how the test knows it was (`route` below restates the host's choice:
enqueue_frames / batch_eligible in capi_batch.cpp, launch_mrfft_range / launch_mrfft_independent in
spectral.hip; its inputs -- frame size, sizes, set_graphs flags, host or device memory and whether any combine
target has two owners, counted by combine_ref -- are all the host reads; nothing observable on the device
tells the kernels apart, and no debug hook was added):
  rfft_pow2    rfft_kernel<K>, Engine.rfft at 512..16384 points (omega_rfft sends these lengths nowhere else)
  small        mrfft_small_kernel: resolutions of 2..256 points (launch_mrfft_range, n < 512)
  res_kernel   mrfft_kernel<K>: frame size 8192, two resolutions sharing a combine target (launch_mrfft)
  res_multi    mrfft_multi_kernel: frame size 8192, disjoint ranges (launch_mrfft_independent); 11 stereo
               frames = 22 channel-frames, 4 per workgroup at 512..2048 points (kMultiThreads /
               small_res_group(n) = 256 / 64): the last workgroup holds 2 frames and 2 padding groups
  res_rf16k    mrfft_rf_kernel<8192>: frame size 16384 with the layout bits of omega_set_graphs set (layout 2:
               batch_eligible is not asked), the 16384-point resolution
  batch_small  batch_multi<256..4096> in batch_kernel: frame size 16384, default layout, disjoint ranges, host
               memory; 22 channel-frames at 8 (512..2048 points), 4 (4096) and 2 (8192) per 512-thread
               workgroup: padding groups at 512..4096 points, and a last role group of 6 of 8
  batch_rf16k  mrfft_rf_body<8192> as role 2 of the same launches
  graph        device memory with graphs on: captured on the first call (while capturing batch_eligible
               returns false: the kernels of res_multi / res_rf16k inside a graph), replayed on the others
  spectra_rf   spectra_rf_body<4096>: Engine.spectra at 8192 points (omega_spectra accepts no other length)
Epilogues: every process_frames call here asks for all magnitudes (mags=True), so every resolution of every
call has a mag_out and takes the full-magnitude epilogue (rfft_magnitudes over all pairs, then magidx; on the
register FFT the per-thread untangle with the magnitudes parked in LDS for the combine). The pair-range and
mag_at epilogues run only for a resolution WITHOUT a magnitude output and emit comb_out alone: those are
tests/test_combine_plans.py's (paths a, b, d). combined=True is on in the 16384-sample calls so that the
combine entries run behind the magnitudes in the same workgroup; it is checked to be finite only.

Signals: any_rfft_ref.designed_pow2(n) = designed(n) (impulses at 0, 1, n//3, n-1, tones, Nyquist, DC, ramp,
noise) plus on-bin tones at bins 1, K/2 - 1, K/2, K/2 + 1, K - 1 (n = 2K: the special slots of untangle,
rfft_magnitudes and thread 0 of spectra_rf_body), at t + NTH q for q in {0, 7}, t in {0, 63, 64, 255} where
the register FFT runs (n >= 8192, NTH = K / 16), and `pair` (two impulses an odd distance apart: |X_k| differs
from bin to bin and between k and K - k, which a single impulse's magnitude does not). A resolution of n
points reads the last n samples of a frame, so each call carries the designed frames of ONE resolution in the
frames' tails behind a noise head and checks that resolution; channel-frame i holds designed frame i mod F, so
channel 0 and channel 1 of every frame differ (frame 0: impulses at 0 and at 1).

Tolerance: per frame and window, dev = the reference's float32 path against X64, max_k |.| / max_k |X64|; a
device output may err by max(4 dev, min(FACTOR[path] dev, cap(n))) + eps32 / 2, cap(n) = eps32 log2(2n), and
always by less than 1e-4; a frame whose windowed product is exactly zero comes back as zero bits; rfft_pow2's
magnitude lies within MAG_ULPS float32 ulps of |.| of its own complex output.

Observed on an MI355X (run with -s), per path over every frame, window and size compared: worst device error
/ worst reference float32 error (both of max |X|) / worst (device error - eps32/2) as a fraction of cap(n):
  rfft_pow2    1.02e-6 / 5.5e-8 / 0.54  (16384, rect, impulse at 16383)
  small        8.2e-8  / 6.5e-8 / 0.04  (16, hamming, tone 7)
  res_kernel, res_multi, batch_small (bitwise the same figures)
               8.38e-7 / 5.5e-8 / 0.47  (8192, hamming, impulse at 8191)
  res_rf16k, batch_rf16k
               7.45e-7 / 5.4e-8 / 0.38  (16384, hamming, impulse at 16383)
  graph        6.56e-7 / 5.4e-8 / 0.46  (1024, blackman, impulse at 1023)
  spectra_rf   4.73e-7 / 5.0e-8 / 0.25  (8192, blackman, impulse at 2730)
Frames the reference gets exactly (dev = 0) come back within 3.2e-8, under the half ulp. rfft_pow2's magnitude
lies within 1.42 ulps of |.| of its complex output (raw v_sqrt_f32 after one fmaf): MAG_ULPS stays 2. Every
FACTOR but `small`'s was widened, by the rule, on frames with dev < eps32: the forcing cases stand beside FACTOR.

Findings.
  1. spectra_rf (fixed here). spectra_rf_body generated its window per thread by a cosine rotation, each value
     within ~2e-7 of the float32 table -- an ABSOLUTE error: under Hann an impulse at sample 1 (w = 1.5e-7) came
     out 1.3e-2 of max |X| off in every bin, past even the 1e-4 bar, impulses at 0 / 8191 under Hamming and
     Blackman likewise, and the impulse at 8191 under Hann, whose product is zero, not as zero. The kernel now
     reads the float32 window table, as mrfft_rf_body does.
  2. small (fixed here). mrfft_small_kernel summed its N products in float32 one after the other: the tone at
     bin 64 of 256 points (rect), which the reference gets exactly, had its own bin 5.72e-7 off (0.48 of cap,
     against a bar of eps32 / 2 at dev = 0). The sums now run in float64 over the float32 twiddles: 8.2e-8.
  3. rfft_pow2 (fixed here). An all-zero frame came back with -0.0 in the complex output (the conjugations of
     the untangle); the kernel adds +0 before the store.
  4. The Stockham BlockFFT paths (rfft_pow2, res_kernel, res_multi, batch_small, graph; fixed here). An impulse
     near the frame's end, whose spectrum is one pure phase ramp, was 0.72 to 1.02 of cap(n) off where the
     register FFT is 0.38 off on the same frame -- 10 to 15 ulps per bin; at (1024, hamming, impulse at 1023)
     the error, 1.40e-6, was past cap(1024) + eps32 / 2 = 1.37e-6 on the three resolution paths. fft_pass
     formed the 15 twiddle powers of a radix-16 butterfly by one multiply chain (w = cmul(w, w1)): the r-th
     power carried r - 1 roundings and r times the rounding of the table's w1. The chain now restarts at
     w^8, read from the table beside w1: at most 0.54 of cap (rfft_pow2 1.77e-6 -> 1.02e-6, the resolution
     paths 1.40e-6 -> 8.38e-7), and the FACTORs fell from 42.5 / 38 to 23 / 16.5.
"""
import numpy as np
import pytest

import any_rfft_ref as A
import combine_ref as CR
from oracle import omega_ref as R
from oracle import signals as S

gpu = pytest.mark.gpu
FS = 48000
MAX_FREQ = 20000
TARGETS = 64
EPS32 = float(np.finfo(np.float32).eps)
SPEC_TOL = 1e-4
MAG_ULPS = 2.0

PATHS = ("rfft_pow2", "small", "res_kernel", "res_multi", "res_rf16k", "batch_small", "batch_rf16k", "graph",
         "spectra_rf")
# FACTOR x dev, never beyond cap(n). 4 is the rule; the wider ones were forced by frames on which the reference's
# float32 spectrum lies within a fraction of an ulp of the largest bin (dev < eps32 = 1.19e-7). Measured on an
# MI355X, the worst (err - eps32/2) / dev per path, rounded up to the next half, with its frame:
#   rfft_pow2    22.6  (16384, rect, impulse at 16383: device 1.02e-6 = 17 x 2^-24, dev 4.21e-8 = 2^-24.5; cap 1.79e-6)
#   res_kernel, res_multi, batch_small, graph
#                16.2  (1024, rect or blackman, impulse at 1023: device 6.56e-7, dev 3.68e-8; cap 1.31e-6)
#   res_rf16k, batch_rf16k
#                14.2  (16384, rect, impulse at 16383: device 6.56e-7, dev 4.21e-8; cap 1.79e-6)
#   spectra_rf   8.49  (8192, blackman, impulse at 8191: device 4.17e-7 = 7 x 2^-24, dev 4.21e-8 = 2^-24.5; cap 1.67e-6)
#   small        0.7   (16, hamming, tone 7): stays 4
FACTOR = {"rfft_pow2": 23.0, "small": 4.0, "res_kernel": 16.5, "res_multi": 16.5, "res_rf16k": 14.5,
          "batch_small": 16.5, "batch_rf16k": 14.5, "graph": 16.5, "spectra_rf": 8.5}

RFFT_SIZES = (512, 1024, 2048, 4096, 8192, 16384)
SMALL_SIZES = (256, 128, 64, 32, 16, 8, 4, 2)
ALL_SIZES = tuple(sorted(set(RFFT_SIZES) | set(SMALL_SIZES)))
DISJOINT = ((20, 200), (200, 1000), (1000, 5000), (5000, 20000))
OVERLAPPING = ((20, 2000), (200, 6000), (1000, 12000), (5000, 20000))
# frame size 8192: every size of 512..8192 points in the first engine or the second
SIZES_8K = ((8192, 4096, 2048, 1024), (4096, 2048, 1024, 512))
CHECK_8K = ((8192, 4096, 2048, 1024), (512,))
# frame size 16384, NORTHSTAR_RESOLUTIONS-shaped: the five batch_multi<K> sizes over the two variants
SIZES_16K = ((16384, 8192, 4096, 2048), (16384, 2048, 1024, 512))
CHECK_16K = ((16384, 8192, 4096, 2048), (1024, 512))
N_FRAMES, N_CHANNELS = 11, 2
N_CF = N_FRAMES * N_CHANNELS
HEAD_SEED = 11
# Not among the inputs: the one (n, window, frame) on which the reference's own float32 magnitude misses the bar
# with FACTOR 4 (numpy's float32 |.| is an ulp off on the frame's largest bin: 1.31e-7 of max |X| against a bar
# of 1.09e-7 at dev = 1.2e-8). The frame is still transformed, in its place among the others; it is not compared.
NOT_AN_INPUT = {(16, "blackman", "ramp")}


def rfft_windows(n):
    return A.WINDOWS if n in (512, 16384) else ("rect", "hann")


def cap(n):
    return EPS32 * np.log2(2.0 * max(n, 1))


def bar_of(dev, n, factor):
    return max(4.0 * dev, min(factor * dev, cap(n))) + 0.5 * EPS32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def small_res_group(n):
    """batch_plan.hpp small_res_group."""
    return max(64, n // 32)


def independent(sizes, ranges):
    """capi_core.cpp res_independent: no combine target with two owners (counted by combine_ref)."""
    cfgs = tuple(R.FFTConfig(tuple(rg), n, max(1, n // 4), 1.0) for n, rg in zip(sizes, ranges))
    _, owners = CR.combine_given({i: np.ones(n // 2 + 1) for i, n in enumerate(sizes)}, cfgs, FS, MAX_FREQ, TARGETS)
    return int(owners.max()) <= 1


def route(W, sizes, indep, flags=0, device=False):
    """{size: path id} of one process_frames call asking for every resolution's magnitudes: the choices of
    omega_process_frames / enqueue_frames / batch_eligible (capi_batch.cpp) and launch_mrfft_range /
    launch_mrfft_independent (spectral.hip), restated. flags: omega_set_graphs (bit 0 graphs, which apply to
    device memory only; bits 1-2 the layout)."""
    graph = bool(flags & 1) and device
    layout3 = not ((flags >> 1) & 3)
    batch = (layout3 and not graph and W == 16384 and indep and sum(n == 16384 for n in sizes) <= 1
             and all(n == 16384 or 512 <= n <= 8192 for n in sizes))
    out = {}
    for n in sizes:
        if batch:
            out[n] = "batch_rf16k" if n == 16384 else "batch_small"
        elif n < 512:
            out[n] = "small"
        elif graph:
            out[n] = "graph"
        elif n == 16384:  # (rf_sizes: the register-FFT kernel, from either launcher)
            out[n] = "res_rf16k"
        else:
            out[n] = "res_multi" if indep else "res_kernel"
    return out


WORST = {}  # path -> [err, dev, (err - eps32/2) / cap, (err - eps32/2) / dev where dev > 0] maxima so far


def check_bins(path, label, n, window, names, X64, dev, cp=None, mag=None):
    """Device complex bins `cp` and / or magnitudes `mag` [F, n//2 + 1] of the frames `names` against the
    float64 expectation X64 with the yardstick dev [F], under FACTOR[path]."""
    w = [0.0, 0.0, -np.inf, 0.0]
    bad = []  # (every frame's figures are printed before the first failure is raised)
    for i, nm in enumerate(names):
        scale = float(np.max(np.abs(X64[i])))
        what = (path, label, n, window, i, nm)
        if (n, window, nm.split(":")[-1]) in NOT_AN_INPUT:
            continue
        if scale == 0.0:  # x * 0 is exact on both sides
            if (cp is not None and bits(cp[i]).any()) or (mag is not None and bits(mag[i]).any()):
                print(f"{path} {label} n={n} {window} {nm}: not zero")
                bad.append(what + ("not zero",))
            continue
        bar = bar_of(dev[i], n, FACTOR[path])
        errs, at = [], []
        if cp is not None:
            assert np.isfinite(cp[i]).all(), what
            e = np.abs(cp[i].astype(np.complex128) - X64[i])
            errs.append(float(e.max()) / scale)
            at.append(int(e.argmax()))
        if mag is not None:
            assert np.isfinite(mag[i]).all(), what
            e = np.abs(mag[i].astype(np.float64) - np.abs(X64[i]))
            errs.append(float(e.max()) / scale)
            at.append(int(e.argmax()))
        err = max(errs)
        ratio = (err - 0.5 * EPS32) / dev[i] if dev[i] else (np.inf if err > 0.5 * EPS32 else 0.0)
        frac = (err - 0.5 * EPS32) / cap(n)
        w = [max(w[0], err), max(w[1], float(dev[i])), max(w[2], frac), max(w[3], ratio if np.isfinite(ratio) else 0.0)]
        print(f"{path} {label} n={n} {window} {nm}: device {err:.2e} of max|X| (bin {at[int(np.argmax(errs))]}), "
              f"reference float32 path {dev[i]:.2e}, bar {bar:.2e}, (err - eps32/2)/dev {ratio:.1f}, /cap {frac:.3f}")
        if not (err <= bar and err < SPEC_TOL):
            bad.append(what + (errs, at, float(dev[i]), bar))
    if cp is not None and mag is not None:
        own = np.abs(cp.astype(np.complex128))
        ulp = np.spacing(own.astype(np.float32)).astype(np.float64)
        off = np.abs(mag.astype(np.float64) - own) / ulp
        print(f"{path} {label} n={n} {window}: magnitude within {off.max():.2f} ulps of |.| of the complex output")
        if not off.max() <= MAG_ULPS:
            bad.append((path, label, n, window, "ulps", float(off.max()), np.unravel_index(off.argmax(), off.shape)))
    acc = WORST.setdefault(path, [0.0, 0.0, -np.inf, 0.0])
    WORST[path] = [max(a, b) for a, b in zip(acc, w)]
    print(f"{path} {label} n={n} {window}: worst device {w[0]:.2e}, reference float32 {w[1]:.2e}, (err - eps32/2)/cap "
          f"{w[2]:.3f}, /dev {w[3]:.1f}; {path} so far {WORST[path][0]:.2e} / {WORST[path][1]:.2e} / "
          f"{WORST[path][2]:.3f} / {WORST[path][3]:.1f}")
    _raise(bad)


def _raise(bad):
    assert not bad, (len(bad), bad[:4])


# ---- CPU: the added signals, the expectation, the yardstick and the routing ----

@pytest.mark.parametrize("n", ALL_SIZES)
def test_added_signals_closed_forms(n):
    """designed_pow2 keeps designed's frames in front, adds tones at every bin the kernels treat specially
    and `pair`; the closed forms of the additions (and the impulses', every window) against np.fft.rfft of
    the float64 signal times the float32 window, 1e-12 of max |X|; `expect` is that transform of the float32
    frame; no two frames are equal and `pair` tells k from K - k."""
    K = n // 2
    base_names, _, base = A.designed(n, "rect")
    sig = dict(A.pow2_signals64(n))
    tones = {int(nm.split("_")[1]) for nm in sig if nm.startswith("tone_")}
    want = {1, K // 2 - 1, K // 2, K // 2 + 1, K - 1}
    if n >= A.REG_FFT_MIN:
        want |= {t + (K // 16) * q for q in (0, 7) for t in (0, 63, 64, 255)}
    assert {b for b in want if 0 <= b <= K} <= tones and max(tones) <= K
    for window in A.WINDOWS:
        names, closed, frames = A.designed_pow2(n, window)
        assert names[:len(base_names)] == base_names and list(sig) == names and names[-1] == "pair"
        np.testing.assert_array_equal(frames[:len(base)], base)
        assert frames.dtype == np.float32 and frames.shape == (len(names), n) and np.isfinite(frames).all()
        w = A.window64(n, window)
        for i, nm in enumerate(names):
            if closed[nm] is None:
                continue
            X = np.fft.rfft(sig[nm] * w)
            tol = 1e-12 * max(float(np.max(np.abs(closed[nm]))), 1e-300)
            assert np.max(np.abs(X - closed[nm])) <= tol, (nm, window)
            if nm.split("_")[0] in ("impulse", "pair"):  # float32 holds these exactly
                assert (frames[i].astype(np.float64) == sig[nm]).all()
                assert np.max(np.abs(A.expect(frames[i], window) - closed[nm])) <= tol, (nm, window)
        assert closed["pair"] is not None and (window != "rect" or all(closed[f"tone_{b}"] is not None for b in tones))
    if n >= 512:
        _, _, frames = A.designed_pow2(n, "rect")
        assert len({f.tobytes() for f in frames}) == len(frames) <= N_CF
        m = np.abs(A.reference_pow2(n, "rect")[0][-1])  # |X| of `pair`
        k = np.arange(1, K // 2)
        assert m.min() > 0.49 and m.max() < 1.51 and np.median(np.abs(m[k] - m[K - k])) > 0.3


@pytest.mark.parametrize("n", ALL_SIZES)
def test_reference_alone_meets_the_bar(n):
    """Every (n, window, frame) the GPU tests use: the reference's float32 path alone, as complex bins and
    as float32 magnitudes, meets the bar with FACTOR 4 and a fourth of 1e-4, and returns exact zeros for a
    frame whose windowed product is zero."""
    for window in A.WINDOWS:
        names, _, frames = A.designed_pow2(n, window)
        X64, dev = A.reference_pow2(n, window)
        assert X64.shape == (len(names), n // 2 + 1)
        for i, nm in enumerate(names):
            X32 = A.yardstick(frames[i], window)
            scale = float(np.max(np.abs(X64[i])))
            if scale == 0.0:
                assert not X32.any() and dev[i] == 0.0, (n, window, nm)
                continue
            bar = bar_of(dev[i], n, 4.0)
            e_c = float(np.max(np.abs(X32.astype(np.complex128) - X64[i]))) / scale
            e_m = float(np.max(np.abs(np.abs(X32).astype(np.float64) - np.abs(X64[i])))) / scale
            assert e_c == dev[i] and e_c <= bar and max(e_c, e_m) < SPEC_TOL / 4, (n, window, nm, e_c, e_m)
            assert (e_m <= bar) == ((n, window, nm) not in NOT_AN_INPUT), (n, window, nm, e_m, bar)
    assert any(not x.any() for x in A.reference_pow2(n, "hann")[0])  # (the zero frames are among the inputs)


def test_tolerance_rule_and_routing():
    assert sorted(FACTOR) == sorted(PATHS) and all(f >= 4.0 for f in FACTOR.values())
    assert bar_of(0.0, 512, 4.0) == 0.5 * EPS32 and bar_of(1e-3, 512, 9.0) == 4.0 * 1e-3 + 0.5 * EPS32
    assert bar_of(1e-8, 512, 9.0) == 9.0 * 1e-8 + 0.5 * EPS32 and cap(512) == 10 * EPS32
    # the partly filled workgroups: mrfft_multi_kernel (256 threads) and batch_kernel (512)
    assert N_CF % (256 // small_res_group(512)) == 2 and all(256 // small_res_group(n) == 4 for n in (512, 1024, 2048))
    assert [N_CF % (512 // small_res_group(n)) for n in (512, 1024, 2048, 4096, 8192)] == [6, 6, 6, 2, 0]
    assert N_CF % 8 == 6 and N_FRAMES != 13
    for sizes in SIZES_8K + SIZES_16K:
        assert independent(sizes, DISJOINT) and not independent(sizes, OVERLAPPING)
    for sizes in SIZES_8K:
        assert set(route(8192, sizes, True).values()) == {"res_multi"}
        assert set(route(8192, sizes, False).values()) == {"res_kernel"}
    for sizes in SIZES_16K:
        r = route(16384, sizes, True)
        assert r[16384] == "batch_rf16k" and {r[n] for n in sizes[1:]} == {"batch_small"}
        assert route(16384, sizes, True, flags=2)[16384] == "res_rf16k"
        assert route(16384, sizes, False)[16384] == "res_rf16k"  # (the other way out of batch_eligible)
        assert set(route(16384, sizes, True, flags=1, device=True).values()) == {"graph"}
        assert route(16384, sizes, True, flags=1, device=False) == r  # (graphs: device memory only)
    assert set(route(512, SMALL_SIZES[:4], False).values()) == {"small"}
    assert {n for s in SIZES_8K for n in s} == {512, 1024, 2048, 4096, 8192} == {n for s in CHECK_8K for n in s}
    assert {n for s in SIZES_16K for n in s if n != 16384} == {512, 1024, 2048, 4096, 8192}
    assert all(set(c) <= set(s) for c, s in zip(CHECK_8K + CHECK_16K, SIZES_8K + SIZES_16K))


# ---- GPU ----

def _engine(sizes, ranges, window, W, flags=0):
    from omega_gpu import Engine, Resolution
    from omega_gpu import _lib as L
    eng = Engine([Resolution(tuple(rg), n, max(1, n // 4), 1.0, window) for n, rg in zip(sizes, ranges)], FS, MAX_FREQ,
                 target_bins=TARGETS, frame_size=W, n_channels=N_CHANNELS, apply_weighting=False)
    if flags:
        eng._check(L.lib().omega_set_graphs(eng._ctx, flags))
    return eng


def _input(n, W):
    """[N_CF, W] float32: channel-frame i = noise head + designed_pow2(n) frame i mod F in its last n samples;
    returns (x, [frame index per channel-frame])."""
    _, _, frames = A.designed_pow2(n)
    idx = [i % len(frames) for i in range(N_CF)]
    assert sorted(set(idx)) == list(range(len(frames)))
    x = np.empty((N_CF, W), np.float32)
    x[:, :W - n] = S.noise(HEAD_SEED, W, 0.2)[:W - n]
    x[:, W - n:] = frames[idx]
    return x, idx


def _check_resolution(path, label, n, window, got, idx):
    names, _, _ = A.designed_pow2(n, window)
    X64, dev = A.reference_pow2(n, window)
    assert got.shape == (N_CF, n // 2 + 1) and got.dtype == np.float32
    check_bins(path, label, n, window, [f"cf{i}:{names[j]}" for i, j in enumerate(idx)], X64[idx], dev[idx], None, got)


def _host_calls(eng, sizes, check, W, window, paths, label, **kw):
    """One host-memory process_frames call per checked resolution, all magnitudes asked for."""
    for n in check:
        x, idx = _input(n, W)
        out = eng.process_frames(x.ravel(), N_FRAMES, N_CHANNELS * W, W, mags=True, **kw)
        if "combined" in out:
            assert np.isfinite(out["combined"]).all()
        _check_resolution(paths[n], label, n, window, out[f"mag{sizes.index(n)}"], idx)


@gpu
@pytest.mark.parametrize("n", RFFT_SIZES)
def test_rfft_pow2(n):
    """Engine.rfft, complex and magnitude output of all designed frames in one call per window."""
    from omega_gpu.engine import utility_engine
    eng = utility_engine(FS)
    for window in rfft_windows(n):
        names, _, frames = A.designed_pow2(n, window)
        X64, dev = A.reference_pow2(n, window)
        mag, cp = eng.rfft(frames, window, magnitude=True, complex_out=True)
        assert mag.shape == cp.shape == X64.shape
        check_bins("rfft_pow2", "rfft", n, window, names, X64, dev, cp, mag)
        m_only, _ = eng.rfft(frames, window, magnitude=True, complex_out=False)
        np.testing.assert_array_equal(bits(m_only), bits(mag))
    eng.close()


@gpu
@pytest.mark.parametrize("window", A.WINDOWS)
def test_small(window):
    """Resolutions of 256..2 points (frame size 512), two engines of four; every range (20, 20000)."""
    for sizes in (SMALL_SIZES[:4], SMALL_SIZES[4:]):
        ranges = ((20, 20000),) * 4
        paths = route(512, sizes, independent(sizes, ranges))
        assert set(paths.values()) == {"small"}
        eng = _engine(sizes, ranges, window, 512)
        _host_calls(eng, sizes, sizes, 512, window, paths, "small", combined=False, lufs=False, true_peak=False)
        eng.close()


@gpu
@pytest.mark.parametrize("window", A.WINDOWS)
@pytest.mark.parametrize("plan", ["res_multi", "res_kernel"])
def test_frame_8192(plan, window):
    """Frame size 8192, resolutions of 512..8192 points: disjoint ranges (mrfft_multi_kernel, a partly
    filled last workgroup at 512..2048 points) and overlapping ones (mrfft_kernel<K> per resolution)."""
    ranges = DISJOINT if plan == "res_multi" else OVERLAPPING
    for sizes, check in zip(SIZES_8K, CHECK_8K):
        paths = route(8192, sizes, independent(sizes, ranges))
        assert set(paths.values()) == {plan}
        eng = _engine(sizes, ranges, window, 8192)
        _host_calls(eng, sizes, check, 8192, window, paths, plan, lufs=False, true_peak=False)
        eng.close()


@gpu
@pytest.mark.parametrize("window", A.WINDOWS)
@pytest.mark.parametrize("variant", [0, 1])
def test_batch_16384(variant, window):
    """Frame size 16384, default layout (one batch_kernel launch: K-weighting, true peak, the 16384-point
    role and the small resolutions' workgroups with padding groups), magnitudes and the combine together."""
    sizes, check = SIZES_16K[variant], CHECK_16K[variant]
    paths = route(16384, sizes, independent(sizes, DISJOINT))
    assert paths[16384] == "batch_rf16k" and {paths[n] for n in sizes[1:]} == {"batch_small"}
    eng = _engine(sizes, DISJOINT, window, 16384)
    _host_calls(eng, sizes, check, 16384, window, paths, f"batch{variant}", combined=True)
    eng.close()


@gpu
@pytest.mark.parametrize("window", A.WINDOWS)
def test_res_rf16k(window):
    """The 16384-point resolution outside the batch layout (layout bits set): mrfft_rf_kernel<8192>."""
    sizes = SIZES_16K[0]
    paths = route(16384, sizes, independent(sizes, DISJOINT), flags=2)
    assert paths[16384] == "res_rf16k"
    eng = _engine(sizes, DISJOINT, window, 16384, flags=2)
    _host_calls(eng, sizes, (16384,), 16384, window, paths, "layout2", combined=True)
    eng.close()


@gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_graph(variant):
    """Device memory with graphs on: the first call captures and launches, the others replay the same graph
    (same pointers: the input tensor is refilled in place); every call's magnitudes against the expectation,
    and a replay of the first input bitwise equal to its first run."""
    import torch
    window = "blackman"
    sizes, check = SIZES_16K[variant], CHECK_16K[variant]
    paths = route(16384, sizes, independent(sizes, DISJOINT), flags=1, device=True)
    assert set(paths.values()) == {"graph"}
    eng = _engine(sizes, DISJOINT, window, 16384, flags=1)
    xd = torch.empty(N_CF * 16384, dtype=torch.float32, device="cuda")
    bufs = None
    first = None
    for n in check + check[:1]:
        x, idx = _input(n, 16384)
        xd.copy_(torch.from_numpy(x.ravel()))
        bufs = eng.process_frames(xd, N_FRAMES, N_CHANNELS * 16384, 16384, mags=True, combined=True, out=bufs)
        torch.cuda.synchronize()
        got = bufs[f"mag{sizes.index(n)}"].cpu().numpy()
        _check_resolution("graph", f"graph{variant}", n, window, got, idx)
        if first is None:
            first = got
    np.testing.assert_array_equal(bits(got), bits(first))
    eng.close()


@gpu
@pytest.mark.parametrize("window", ["hann", "blackman", "hamming", "rect"])
def test_spectra_rf(window):
    """Engine.spectra at 8192 points, magnitudes only, then with the chromagram on the same frames: the
    magnitudes per bin, and bitwise equal between the two calls."""
    from omega_gpu import Engine, Resolution
    n = 8192
    eng = Engine([Resolution((20, 20000), n, 2048, 1.0)], FS, MAX_FREQ, 512)
    names, _, frames = A.designed_pow2(n, window)
    X64, dev = A.reference_pow2(n, window)
    out = eng.spectra(frames, window, bands=None, chroma=False, mags=True)
    assert set(out) == {"mag"} and out["mag"].shape == X64.shape
    check_bins("spectra_rf", "spectra", n, window, names, X64, dev, None, out["mag"])
    both = eng.spectra(frames, window, bands=None, chroma=True, mags=True)
    assert set(both) == {"mag", "chroma"}
    np.testing.assert_array_equal(bits(both["mag"]), bits(out["mag"]))
    eng.close()


@gpu
@pytest.mark.parametrize("window", ["hann", "blackman"])
def test_spectra_rf_lds_magnitudes(window):
    """The magnitude output is stored from registers; the band and chroma phases read a second copy, the
    magc array in LDS (its own pair store, thread 0's extra bins). One-bin MAX bands (band i = bin a + i,
    no scale) return that copy: bitwise the magnitude output, bin by bin, nine tables of at most 512 bands."""
    from omega_gpu import Engine, Resolution
    from omega_gpu import _lib as L
    from omega_gpu.engine import BandTable
    n = 8192
    eng = Engine([Resolution((20, 20000), n, 2048, 1.0)], FS, MAX_FREQ, 512)
    _, _, frames = A.designed_pow2(n, window)
    mag = eng.spectra(frames, window, bands=None, chroma=False, mags=True)["mag"]
    for a in range(0, n // 2 + 1, 512):
        k = np.arange(a, min(a + 512, n // 2 + 1))
        bt = BandTable(eng, L.BANDS_MAX, k, k + 1, len(k), n // 2 + 1)
        out = eng.spectra(frames, window, bands=bt, chroma=False, mags=True)
        np.testing.assert_array_equal(bits(out["mag"]), bits(mag))
        np.testing.assert_array_equal(bits(out["bands"]), bits(mag[:, k]), err_msg=f"{window} bins {a}..{k[-1]}")
    eng.close()
