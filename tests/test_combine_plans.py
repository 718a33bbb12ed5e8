"""The combine plan, target bin by target bin, on overlapping and off-default plans.

Every implementation of the combine step (mrfft_frame's direct, pair-range and all-magnitudes variants,
mrfft_rf_body's combine-only, parked-magnitudes and run_low paths, mrfft_small_kernel, mrfft_multi_kernel,
the batch kernel's resolution roles and the stand-alone combine_kernel) applies one host-built CombEnt plan
(capi_core.cpp build_spectral_tables). The plans below give targets 0 to 4 owners, end at Nyquist, start at
0 Hz, skip a resolution with a single in-range bin, leave most targets unowned, use 44.1 and 96 kHz weight
tables and move target_bins to both sides of the direct / pair-range switch; the paths cover host and
device memory, strided frames, magnitude outputs for all / one / no resolution, meters (the batch kernel
or, with overlapping owners, its fallback), pipelined meters, apply_weighting=False, omega_combine and the
MultiResolutionFFT facade.

Reference: tests/combine_ref.py, a float64 restatement of the reference's process_audio_chunk and
combine_results_optimized. Frames are S.noise(seed, W, 0.2): comparable magnitude in every bin, so the bar
is per bin. With rms the root mean square of the reference over the owned targets of a channel-frame,
every owned target must satisfy |got - ref| <= SPEC_TOL * rms (SPEC_TOL = 1e-4, the project's spectra bar,
per bin against rms instead of normwise against the maximum); unowned targets must be exactly 0.0; every
weighted magnitude output is held to the same bar against its resolution's own rms. omega_combine on given
float32 magnitudes in [0.5, 1.5] is held to rtol 4e-6 per target (fewer than ten float32 roundings of 6e-8,
inputs within a factor of 3 of each other: no cancellation). Every combined output is handed in through
out= prefilled with NaN, so a target nobody writes fails. The CPU tests pin each plan's owner histogram and
hold the float32 oracle to the same bar (it measures 1e-7 to 1.3e-6 of rms: a hundredfold margin).

Worst measured err / rms per plan and path on an MI355X (bar 1e-4; "m" columns: the magnitude outputs; g:
the worst relative error of omega_combine, bar 4e-6; no test failed, no fix was needed):

        a(1)    a(5)    b       c       c m     d       d m     e       f       g       h
  P1    8.6e-7  1.5e-6  1.2e-6  1.2e-6  1.7e-6  1.5e-6  1.5e-6  1.3e-6  1.0e-6  1.3e-7  1.2e-6
  P2    5.3e-7  1.9e-6  1.3e-6  2.4e-6  1.8e-6  1.2e-6  8.1e-7  -       -       1.6e-7  2.1e-6
  P3    5.6e-7  1.2e-6  2.1e-6  1.5e-6  1.4e-6  1.4e-6  1.5e-6  -       -       -       -
  P4    2.1e-6  4.6e-6  4.1e-6  3.9e-6  1.4e-6  4.7e-6  1.7e-6  -       1.4e-6  1.5e-7  2.8e-6
  P5a   7.3e-7  1.2e-6  1.1e-6  9.6e-7  1.5e-6  1.2e-6  1.5e-6  1.0e-6  -       -       -
  P5b   2.4e-6  3.3e-6  4.1e-6  3.2e-6  1.6e-6  2.4e-6  1.6e-6  3.6e-6  -       -       -
  P6    6.4e-7  3.7e-7  3.4e-7  2.7e-6  1.7e-6  4.7e-7  1.5e-6  1.6e-6  -       -       -

(e on P1 with pipelined meters: 1.1e-6 and 1.5e-6 for the two calls; h is the worst of the combine kernel,
the cached in-launch combine and the facade's magnitudes.) A host-memory call returns its outputs through
the context's staging buffers, so there the NaN prefill cannot show an unwritten target; the device paths do.
"""
import functools

import numpy as np
import pytest

import combine_ref as CR
from oracle import omega_ref as R
from oracle import signals as S

gpu = pytest.mark.gpu
SPEC_TOL = 1e-4       # the project's spectra bar, applied per bin against the owned targets' rms
COMBINE_RTOL = 4e-6   # omega_combine on given float32 magnitudes

NS = [((20, 200), 16384, 1024, 1.5), ((200, 1000), 8192, 512, 1.2), ((1000, 5000), 4096, 256, 1.0),
      ((5000, 20000), 1024, 256, 1.5)]
# name: (resolutions as (range, N, hop, weight), fs, max_freq, T, W)
PLANS = {
    "P1": ([((20, 2000), 16384, 1024, 1.5), ((200, 6000), 8192, 512, 1.2), ((1000, 12000), 4096, 256, 1.0),
            ((5000, 20000), 1024, 256, 1.5)], 48000, 20000, 512, 16384),
    "P2": ([((20, 3000), 2048, 512, 1.5), ((1000, 24000), 512, 128, 1.2), ((500, 8000), 256, 64, 1.0),
            ((0, 24000), 1024, 256, 0.7)], 48000, 24000, 333, 2048),
    "P3": ([((100, 400), 4096, 1024, 1.5), ((90, 100), 512, 128, 1.2), ((2000, 3000), 1024, 256, 1.0)],
           48000, 20000, 512, 4096),
    "P4": ([((20, 2500), 8192, 512, 1.5), ((150, 9000), 2048, 512, 1.2), ((4000, 18000), 512, 256, 1.0)],
           44100, 18000, 1024, 8192),
    "P5a": (NS, 48000, 20000, 64, 16384),
    "P5b": (NS, 48000, 20000, 4096, 16384),
    "P6": (NS, 96000, 20000, 2, 16384),
}
# targets with 0, 1, 2, ... owners
HISTOGRAMS = {
    "P1": [1, 210, 249, 52],
    "P2": [0, 1, 228, 76, 28],
    "P3": [479, 33],
    "P4": [2, 604, 418],
    "P5a": [1, 63],
    "P5b": [5, 4091],
    "P6": [1, 1],
}
ALL = list(PLANS)
OVERLAPPING = ["P1", "P2", "P4"]
W16K = [n for n in ALL if PLANS[n][4] == 16384]
SEED0 = {n: 1000 * (k + 1) for k, n in enumerate(ALL)}  # a seed range per plan


def _configs(name):
    return tuple(R.FFTConfig(tuple(rg), n, hop, w) for rg, n, hop, w in PLANS[name][0])


def _frame(name, seed):
    return S.noise(seed, PLANS[name][4], 0.2)


@functools.lru_cache(maxsize=None)
def _ref(name, seed, weighting=True):
    """(combined, owners, {i: magnitudes}) of the plan's frame `seed`: computed once, shared, read-only."""
    _, fs, mf, T, _ = PLANS[name]
    comb, owners, mags = CR.reference(_frame(name, seed), _configs(name), fs, mf, T, weighting)
    for a in (comb, owners, *mags.values()):
        a.flags.writeable = False
    return comb, owners, mags


def _check_combined(name, path, got, seeds, weighting=True):
    """got [n_cf, T] against the reference of each channel-frame's seed; returns the worst err / rms."""
    got = np.asarray(got)
    T = PLANS[name][3]
    assert got.shape == (len(seeds), T) and got.dtype == np.float32
    worst = 0.0
    for cf, seed in enumerate(seeds):
        ref, owners, _ = _ref(name, seed, weighting)
        owned = owners > 0
        free = got[cf][~owned]
        assert np.all(free == 0.0), (name, path, cf, "unowned targets", np.where(~owned)[0][free != 0.0][:8])
        err = np.abs(got[cf][owned].astype(np.float64) - ref[owned]) / CR.owned_rms(ref, owners)
        bad = ~(err <= SPEC_TOL)  # (a NaN is bad)
        worst = max(worst, float(np.max(err)) if not np.isnan(err).any() else np.inf)
        assert not bad.any(), (name, path, cf, "targets", np.where(owned)[0][bad][:8], err[bad][:8])
    print(f"combine-plans {name} {path} combined worst err/rms {worst:.3e}")
    return worst


def _check_mags(name, path, out, seeds, sel, weighting=True):
    worst = 0.0
    for r in sel:
        got = np.asarray(out[f"mag{r}"])
        for cf, seed in enumerate(seeds):
            ref = _ref(name, seed, weighting)[2][r]
            assert got[cf].shape == ref.shape
            err = np.abs(got[cf].astype(np.float64) - ref) / CR.owned_rms(ref)
            bad = ~(err <= SPEC_TOL)
            worst = max(worst, float(np.max(err)) if not np.isnan(err).any() else np.inf)
            assert not bad.any(), (name, path, cf, r, "bins", np.where(bad)[0][:8], err[bad][:8])
    print(f"combine-plans {name} {path} magnitudes worst err/rms {worst:.3e}")
    return worst


# ---------------------------------------------------------------------------------------------
# CPU: the plans are what they are meant to be, and the reference and the bar hold for the oracle
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_owner_histogram(name):
    _, owners, mags = _ref(name, SEED0[name])
    assert np.bincount(owners).tolist() == HISTOGRAMS[name]
    assert sorted(mags) == list(range(len(PLANS[name][0])))
    if name == "P3":  # the 512-point resolution has the single in-range bin 93.75 Hz: it owns nothing
        f = np.fft.rfftfreq(512, 1 / 48000)
        assert f[(f >= 90) & (f <= 100)].tolist() == [93.75]
        sub, own1 = CR.combine_given({1: mags[1]}, _configs(name), 48000, 20000, 512)
        assert not own1.any() and not sub.any()


@pytest.mark.parametrize("name", ALL)
def test_oracle_inside_bar(name):
    """The float32 oracle R.combine(R.mrfft_frame(...)) against the float64 reference under the per-bin
    bar (three seeds per plan; weighting off too on the plans path f uses): validates reference and bar."""
    cfgs = _configs(name)
    _, fs, mf, T, _ = PLANS[name]
    for weighting in (True, False) if name in ("P1", "P4") else (True,):
        for seed in (SEED0[name], SEED0[name] + 1, SEED0[name] + 2):
            got, tgt = R.combine(R.mrfft_frame(_frame(name, seed), cfgs, fs, weighting), cfgs, fs, mf, T)
            np.testing.assert_array_equal(tgt, CR.targets(fs, mf, T))
            _check_combined(name, "oracle", got[None], [seed], weighting)


@pytest.mark.parametrize("name", OVERLAPPING)
def test_combine_given_matches_oracle_on_subsets(name):
    """combine_given on given float32 magnitudes, all resolutions and without resolution 1, against the
    oracle's float32 combine of the same values (the bar omega_combine is held to)."""
    cfgs = _configs(name)
    _, fs, mf, T, _ = PLANS[name]
    rng = np.random.default_rng(SEED0[name] + 7)
    mags = {i: rng.uniform(0.5, 1.5, c.fft_size // 2 + 1).astype(np.float32) for i, c in enumerate(cfgs)}
    for keep in (list(mags), [i for i in mags if i != 1]):
        sub = {i: mags[i] for i in keep}
        ref, owners = CR.combine_given(sub, cfgs, fs, mf, T)
        got, _ = R.combine(sub, cfgs, fs, mf, T)
        assert np.all(got[owners == 0] == 0.0)
        np.testing.assert_allclose(got[owners > 0], ref[owners > 0], rtol=COMBINE_RTOL, atol=0)
    full = CR.combine_given(mags, cfgs, fs, mf, T)[1]
    assert (full - owners).max() == 1  # dropping resolution 1 takes an owner away somewhere


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

def _engine(name, C, **kw):
    from omega_gpu import Engine, Resolution
    res, fs, mf, T, W = PLANS[name]
    return Engine([Resolution(tuple(rg), n, hop, w) for rg, n, hop, w in res], fs, mf, target_bins=T,
                  frame_size=W, n_channels=C, **kw)


def _seeds(name, path, F, C, call=0):
    """Frame-major seeds [F * C] (channel-frame f * C + c), distinct per plan, path, call, frame, channel."""
    base = SEED0[name] + 100 * (ord(path) - ord("a") + 1) + 40 * call
    return [base + f * C + c for f in range(F) for c in range(C)]


def _packed(name, seeds, F, C, frame_stride, chan_stride):
    """Flat float32 input: frame f, channel c at f * frame_stride + c * chan_stride; NaN between frames."""
    W = PLANS[name][4]
    x = np.full((F - 1) * frame_stride + (C - 1) * chan_stride + W, np.nan, np.float32)
    for f in range(F):
        for c in range(C):
            o = f * frame_stride + c * chan_stride
            x[o:o + W] = _frame(name, seeds[f * C + c])
    return x


def _device_call(name, eng, path, F, C, call=0, **kw):
    """One strided device-memory process_frames call with a NaN-prefilled combined output; returns
    (outputs as host arrays, seeds)."""
    import torch
    W, T = PLANS[name][4], PLANS[name][3]
    seeds = _seeds(name, path, F, C, call)
    fstride, cstride = C * W + 6 * C + 10, W + 6  # even, and the frames are not packed
    xd = torch.from_numpy(_packed(name, seeds, F, C, fstride, cstride)).cuda()
    comb = torch.full((F * C, T), float("nan"), dtype=torch.float32, device="cuda")
    out = eng.process_frames(xd, F, fstride, cstride, out={"combined": comb}, **kw)
    return out, seeds, xd


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@gpu
@pytest.mark.parametrize("name", ALL)
def test_a_host_combined_only(name):
    """Host numpy input, combined only: 1 frame, then 5 frames (a partly filled mrfft_multi_kernel
    workgroup). With overlapping owners the outputs cannot be zero-copy (o[t] += v reads back)."""
    W, T = PLANS[name][4], PLANS[name][3]
    eng = _engine(name, 1)
    for call, F in enumerate((1, 5)):
        seeds = _seeds(name, "a", F, 1, call)
        x = _packed(name, seeds, F, 1, W, W)
        comb = np.full((F, T), np.nan, np.float32)
        out = eng.process_frames(x, F, W, W, lufs=False, true_peak=False, out={"combined": comb})
        assert out["combined"] is comb and set(out) == {"combined"}
        _check_combined(name, f"a{F}", comb, seeds)
    eng.close()


@gpu
@pytest.mark.parametrize("name", ALL)
def test_b_device_combined_only_strided(name):
    eng = _engine(name, 2)
    out, seeds, _ = _device_call(name, eng, "b", 3, 2, lufs=False, true_peak=False)
    _check_combined(name, "b", _host(out)["combined"], seeds)
    eng.close()


@gpu
@pytest.mark.parametrize("name", ALL)
def test_c_device_all_magnitudes(name):
    eng = _engine(name, 2)
    out, seeds, _ = _device_call(name, eng, "c", 3, 2, lufs=False, true_peak=False, mags=True)
    out = _host(out)
    _check_combined(name, "c", out["combined"], seeds)
    _check_mags(name, "c", out, seeds, range(len(PLANS[name][0])))
    eng.close()


D_RES = {"P3": 2}  # (P3's resolution 1 owns nothing; its magnitudes are checked by path c)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_d_device_one_magnitude(name):
    """combined plus the magnitudes of one resolution: mag_out set and unset within one call."""
    r = D_RES.get(name, 1)
    eng = _engine(name, 2)
    out, seeds, _ = _device_call(name, eng, "d", 3, 2, lufs=False, true_peak=False, mags=[r])
    out = _host(out)
    assert set(out) == {"combined", f"mag{r}"}
    _check_combined(name, "d", out["combined"], seeds)
    _check_mags(name, "d", out, seeds, [r])
    eng.close()


@gpu
@pytest.mark.parametrize("name", W16K)
def test_e_device_with_meters(name):
    """16384-sample frames with meters: the independent plans take the batch kernel, P1 (overlapping
    owners) its fallback; the combined output is the same and the meters are finite."""
    eng = _engine(name, 2)
    out, seeds, _ = _device_call(name, eng, "e", 3, 2, meters=True)
    out = _host(out)
    _check_combined(name, "e", out["combined"], seeds)
    assert out["meters"].shape == (6, 5) and np.isfinite(out["meters"]).all()
    assert np.isfinite(out["lufs_inst"]).all() and np.isfinite(out["true_peak_db"]).all()
    eng.close()


@gpu
def test_e_pipelined_meters_overlapping_plan():
    """P1 with set_meter_pipelining: two calls, flush_meters, synchronize; both calls' outputs."""
    eng = _engine("P1", 2)
    eng.set_meter_pipelining(True)
    calls = [_device_call("P1", eng, "e", 1, 2, call=k + 1, meters=True) for k in range(2)]
    eng.flush_meters()
    eng.synchronize()
    for k, (out, seeds, _) in enumerate(calls):
        out = _host(out)
        _check_combined("P1", f"e-pipe{k}", out["combined"], seeds)
        assert np.isfinite(out["meters"]).all()
    eng.close()


@gpu
@pytest.mark.parametrize("name", ["P1", "P4"])
def test_f_unweighted(name):
    eng = _engine(name, 2, apply_weighting=False)
    out, seeds, _ = _device_call(name, eng, "f", 3, 2, lufs=False, true_peak=False)
    _check_combined(name, "f", _host(out)["combined"], seeds, weighting=False)
    eng.close()


@gpu
@pytest.mark.parametrize("name", OVERLAPPING)
def test_g_combine_kernel_given_magnitudes(name):
    """Engine.combine (combine_kernel) on given float32 magnitudes in [0.5, 1.5], 3 channel-frames: all
    resolutions, then without resolution 1, against the float64 combine of the same values."""
    cfgs = _configs(name)
    _, fs, mf, T, _ = PLANS[name]
    n_cf = 3
    rng = np.random.default_rng(SEED0[name] + 700)
    mags = {i: rng.uniform(0.5, 1.5, (n_cf, c.fft_size // 2 + 1)).astype(np.float32) for i, c in enumerate(cfgs)}
    eng = _engine(name, 1)
    worst = 0.0
    for keep in (list(mags), [i for i in mags if i != 1]):
        got = eng.combine({i: mags[i] for i in keep}, n_cf)
        assert got.shape == (n_cf, T) and got.dtype == np.float32
        for cf in range(n_cf):
            ref, owners = CR.combine_given({i: mags[i][cf] for i in keep}, cfgs, fs, mf, T)
            owned = owners > 0
            assert np.all(got[cf][~owned] == 0.0), (name, keep, cf)
            rel = np.abs(got[cf][owned] - ref[owned]) / np.abs(ref[owned])
            worst = max(worst, float(rel.max()))
            assert np.all(rel <= COMBINE_RTOL), (name, keep, cf, np.where(owned)[0][~(rel <= COMBINE_RTOL)][:8])
    print(f"combine-plans {name} g combine_kernel worst relative error {worst:.3e}")
    eng.close()


@gpu
@pytest.mark.parametrize("name", OVERLAPPING)
def test_h_facade(name):
    """MultiResolutionFFT with the plan's configs: a chunk, its results combined as returned and as copies
    (copies never match the cached launch: the combine kernel), then a further chunk whose own launch
    formed the combine at the target last asked for, returned from the cache."""
    from omega_gpu.multi_resolution_fft import FFTConfig, MultiResolutionFFT
    res, fs, mf, T, W = PLANS[name]
    m = MultiResolutionFFT(fs, max_freq=mf)
    m.configs = [FFTConfig(*c) for c in res]
    m._setup_windows(); m._setup_buffers(); m._setup_frequency_arrays(); m._setup_working_arrays()
    seeds = _seeds(name, "h", 2, 1)
    r0 = m.process_audio_chunk(_frame(name, seeds[0]))
    assert sorted(r0) == list(range(len(res)))
    copies = {i: r._replace(magnitude=r.magnitude.copy()) for i, r in r0.items()}
    for label, given in (("h-first", r0), ("h-kernel", copies)):  # (P4's T is the facade's default target:
        c0, t0 = m.combine_results_optimized(given, T)            # its first combine is the launch's own)
        np.testing.assert_array_equal(t0, np.linspace(0, mf, T))
        _check_combined(name, label, c0[None], seeds[:1])
    _check_mags(name, "h", {f"mag{i}": r.magnitude[None] for i, r in r0.items()}, seeds[:1], sorted(r0))
    r1 = m.process_audio_chunk(_frame(name, seeds[1]))
    assert m._last is not None and m._last[2] == T  # formed in the chunk's launch
    c1, t1 = m.combine_results_optimized(r1, T)
    np.testing.assert_array_equal(t1, np.linspace(0, mf, T))
    _check_combined(name, "h-cached", c1[None], seeds[1:])
    m.cleanup()
