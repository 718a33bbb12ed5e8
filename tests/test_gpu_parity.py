"""Parity of the HIP path (through the C ABI, via the omega_gpu facades) against the reference's golden
vectors and the oracle. Tolerances are the north-star bars (BASELINE.json): spectra <= 1e-4 normwise
(|a-b|_inf / max|b| per frame and resolution), LUFS <= 0.1 LU; true peak <= 0.01 dB."""
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, normwise
from oracle import omega_ref as R
from oracle import signals as S

pytestmark = pytest.mark.gpu
FS = 48000
SPEC_TOL = 1e-4   # north star: <= 1e-4 relative on float32 spectra (normwise)
LU_TOL = 0.1      # north star: <= 0.1 LU on LUFS
TP_TOL_DB = 0.01  # true peak (float32 FFT on both sides)


@pytest.fixture(scope="module")
def mr():
    return load_golden("mrfft")


@pytest.fixture(scope="module")
def me():
    return load_golden("meters")


def _mrfft(configs=None):
    from omega_gpu.multi_resolution_fft import MultiResolutionFFT, FFTConfig
    m = MultiResolutionFFT(FS)
    if configs is not None:
        m.configs = [FFTConfig(*c) for c in configs]
        m._setup_windows(); m._setup_buffers(); m._setup_frequency_arrays(); m._setup_working_arrays()
    return m


NS = [((20, 200), 16384, 1024, 1.5), ((200, 1000), 8192, 512, 1.2), ((1000, 5000), 4096, 256, 1.0),
      ((5000, 20000), 1024, 256, 1.5)]


def test_native_library_is_the_path():
    import omega_gpu
    assert omega_gpu.lib().omega_version().startswith(b"omega-mi355x")


@pytest.mark.parametrize("name", ["sine1k_2048", "noise_2048", "triad_4096", "comp_4096", "silence_4096",
                                  "sine50_8192"])
def test_mrfft_golden_default(mr, name):
    """The default resolutions against the reference's golden magnitudes and combines. SPEC_TOL is the
    north-star bar only: the float32-accuracy comparison of every resolution kernel, bin by bin on designed
    signals, is tests/test_pow2_rfft_bins.py (eps32 log2(2N) at most)."""
    m = _mrfft()
    x = mr[f"{name}/x"]
    res = m.process_audio_chunk(x)
    assert sorted(res) == list(mr[f"{name}/res"])
    for i, r in res.items():
        assert r.magnitude.dtype == np.float32 and r.config_index == i
        g = mr[f"{name}/mag{i}"]
        if np.max(g) == 0:
            assert np.max(np.abs(r.magnitude)) == 0
        else:
            assert normwise(r.magnitude, g) < SPEC_TOL, (i, normwise(r.magnitude, g))
        np.testing.assert_array_equal(r.frequencies, np.fft.rfftfreq(m.configs[i].fft_size, 1 / FS))
    raw = _mrfft().process_audio_chunk(x, apply_weighting=False)
    for i, r in raw.items():
        g = mr[f"{name}/raw{i}"]
        if np.max(g) > 0:
            assert normwise(r.magnitude, g) < SPEC_TOL
    for T in (512, 1024):
        c, t = m.combine_results_optimized(res, target_bins=T)
        np.testing.assert_array_equal(t, mr[f"{name}/tgt{T}"])
        g = mr[f"{name}/comb{T}"]
        assert c.dtype == np.float32 and c.shape == (T,)
        assert (np.max(np.abs(c)) == 0) if np.max(g) == 0 else normwise(c, g) < SPEC_TOL


@pytest.mark.parametrize("k", [0, 1, 2])
def test_mrfft_golden_northstar(mr, k):
    m = _mrfft(NS)
    res = m.process_audio_chunk(mr[f"ns{k}/x"])
    assert sorted(res) == [0, 1, 2, 3]
    for i in range(4):
        assert normwise(res[i].magnitude, mr[f"ns{k}/mag{i}"]) < SPEC_TOL
    c, _ = m.combine_results_optimized(res, 512)
    assert normwise(c, mr[f"ns{k}/comb512"]) < SPEC_TOL


def test_mrfft_combine_reuse_needs_unmodified_results(mr):
    """process_audio_chunk forms the 1024-target combine in the same launch and combine_results_optimized
    returns it only for exactly those results, unmodified: a magnitude changed in place, or a dict from
    elsewhere, is combined on the device from the values given (as the reference combines whatever it
    is handed)."""
    m = _mrfft()
    x = mr["triad_4096/x"]
    res = m.process_audio_chunk(x)
    c0, _ = m.combine_results_optimized(res, 1024)
    assert normwise(c0, mr["triad_4096/comb1024"]) < SPEC_TOL
    res[1].magnitude[:] *= 3.0
    c1, _ = m.combine_results_optimized(res, 1024)
    fresh = _mrfft()
    c2, _ = fresh.combine_results_optimized(res, 1024)  # (no cached launch: the combine kernel)
    np.testing.assert_array_equal(c1, c2)
    assert normwise(c1, c0) > 1e-3
    copied = {i: r._replace(magnitude=r.magnitude.copy()) for i, r in m.process_audio_chunk(x).items()}
    c3, _ = m.combine_results_optimized(copied, 1024)
    np.testing.assert_array_equal(c3, fresh.combine_results_optimized(copied, 1024)[0])


def test_mrfft_combine_reuse_follows_target_bins(mr):
    """The app's call pair (omega4_main.py:707-717: a float64 Hann-windowed frame, then the combine at
    target_bins = its display bars): the first combine at 512 targets runs on the device from the values
    given and makes every later chunk form the 512-target combine in its own launch; that cached result
    is returned only for the unmodified results of the last chunk, equals the combine kernel's, and
    follows the reference to SPEC_TOL. A max_freq change after the chunk invalidates it."""
    m = _mrfft()
    x = mr["triad_4096/x"]
    x64 = np.asarray(x, np.float64)
    res = m.process_audio_chunk(x64)
    c0, f0 = m.combine_results_optimized(res, 512)  # (the combine kernel; the target is now 512)
    assert normwise(c0, mr["triad_4096/comb512"]) < SPEC_TOL
    np.testing.assert_allclose(f0, mr["triad_4096/tgt512"])
    res = m.process_audio_chunk(x64)
    assert m._last is not None and m._last[2] == 512  # formed in the chunk's launch
    c1, f1 = m.combine_results_optimized(res, 512)
    assert normwise(c1, mr["triad_4096/comb512"]) < SPEC_TOL
    np.testing.assert_array_equal(f1, f0)
    fresh = _mrfft()
    c2, _ = fresh.combine_results_optimized(res, 512)
    np.testing.assert_allclose(c1, c2, rtol=1e-6, atol=1e-7)
    res[2].magnitude[:] *= 2.0  # modified: combined from the values given
    c3, _ = m.combine_results_optimized(res, 512)
    np.testing.assert_array_equal(c3, fresh.combine_results_optimized(res, 512)[0])
    res = m.process_audio_chunk(x64)
    m.max_freq = 16000.0  # configuration changed after the chunk: no stale reuse
    c4, f4 = m.combine_results_optimized(res, 512)
    assert f4[-1] == 16000.0
    np.testing.assert_array_equal(c4, _mrfft_maxf(16000.0).combine_results_optimized(res, 512)[0])


def _mrfft_maxf(mf):
    from omega_gpu.multi_resolution_fft import MultiResolutionFFT
    return MultiResolutionFFT(FS, max_freq=mf)


SMALL = [((20, 2000), 256, 128, 1.5), ((200, 6000), 128, 64, 1.2), ((1000, 12000), 64, 32, 1.0),
         ((5000, 20000), 512, 256, 1.5)]


def test_mrfft_small_sizes_golden():
    """Resolutions below 512 points (mrfft_small_kernel: direct sums over the N-point twiddle table)
    mixed with a 512-point one, against the reference's MultiResolutionFFT."""
    g = load_golden("mrfft_small")
    for name in ("sine", "noise", "triad"):
        m = _mrfft(SMALL)
        res = m.process_audio_chunk(g[f"{name}/x"])
        assert sorted(res) == list(g[f"{name}/res"])
        for i, r in res.items():
            assert normwise(r.magnitude, g[f"{name}/mag{i}"]) < SPEC_TOL, (name, i)
        c, _ = m.combine_results_optimized(res, 512)
        assert normwise(c, g[f"{name}/comb512"]) < SPEC_TOL


def test_mrfft_stream_layout(mr):
    """One instance fed 512-sample chunks: CircularBuffer availability and contents."""
    m = _mrfft()
    x = mr["stream/x"]
    for c in range(24):
        r = m.process_audio_chunk(x[c * 512:(c + 1) * 512])
        assert sum(1 << i for i in r) == mr["stream/resmask"][c]
        comb = m.combine_results_optimized(r, 512)[0] if r else np.zeros(512, np.float32)
        g = mr["stream/comb512"][c]
        assert (np.max(np.abs(comb)) == 0) if np.max(g) == 0 else normwise(comb, g) < SPEC_TOL
    for i in r:
        assert normwise(r[i].magnitude, mr[f"stream/mag{i}"]) < SPEC_TOL


def test_mrfft_empty_chunk():
    m = _mrfft()
    assert m.process_audio_chunk(np.zeros(0, np.float32)) == {}
    z, t = m.combine_results_optimized({}, 512)
    assert z.shape == (512,) and not z.any() and t[-1] == 20000


@pytest.mark.parametrize("name", ["sine2048", "hann2048_f64", "comp4800", "square480"])
def test_k_weighting_golden(me, name):
    from omega_gpu.professional_meters import ProfessionalMetering
    pm = ProfessionalMetering(FS)
    x = me[f"kw/{name}/x"]
    y = pm.apply_k_weighting(x)
    g = me[f"kw/{name}/y"]
    assert y.dtype == np.float64
    # omega_weighting runs scipy's float64 filtfilt (weight64.hip); what remains is the float32 rounding
    # of the returned signal (the ABI's output type) and of a float64 input frame
    assert normwise(y, g) < 1e-6, normwise(y, g)
    ms_dev, ms_ref = np.mean(y ** 2), np.mean(g ** 2)
    assert abs(10 * np.log10(ms_dev) - 10 * np.log10(ms_ref)) < 1e-4
    assert abs(pm.calculate_true_peak(x) - me[f"kw/{name}/tp"]) < TP_TOL_DB


def test_k_weighting_coefficients(me):
    """k_weighting_filter and create_k_weighting_filter (professional_meters.py:48-72) against the
    reference's scipy coefficients (golden), the unused shelf gain included."""
    from omega_gpu.professional_meters import ProfessionalMetering
    pm = ProfessionalMetering(FS)
    for kf in (pm.k_weighting_filter, pm.create_k_weighting_filter()):
        for k, g in (("hp_b", "coef/hp_b"), ("hp_a", "coef/hp_a"), ("shelf_b", "coef/sh_b"), ("shelf_a", "coef/sh_a")):
            np.testing.assert_allclose(kf[k], me[g], rtol=1e-12, atol=1e-15)
        assert kf["shelf_gain"] == 10 ** (4.0 / 20)


@pytest.mark.parametrize("name", ["cfg2L", "sine2048", "low50_4096", "silence", "steps1024", "square1024"])
def test_meter_sequences_facade(me, name):
    """calculate_lufs called frame by frame (the panel's call pattern, professional_meters.py:348-351)."""
    from omega_gpu.professional_meters import ProfessionalMetering
    pm = ProfessionalMetering(FS)
    frames = me[f"{name}/x"]
    agg = me[f"{name}/agg"]
    for f, x in enumerate(frames):
        d = pm.calculate_lufs(x)
        assert set(d) == {"momentary", "short_term", "integrated", "range", "true_peak"}
        got = np.array([d[k] for k in ("momentary", "short_term", "integrated", "range", "true_peak")])
        assert np.all(np.abs(got[:4] - agg[f, :4]) < LU_TOL), (f, got, agg[f])
        assert abs(got[4] - agg[f, 4]) < TP_TOL_DB, (f, got[4], agg[f, 4])
    assert d is pm.current_lufs


@pytest.mark.parametrize("name", ["cfg2L", "sine2048", "steps1024"])
def test_meter_instantaneous(me, name):
    from omega_gpu import Engine, Resolution
    frames = me[f"{name}/x"]
    e = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)
    _, li = e.k_weighting_scan(frames, weighted=False)  # the batch kernel's float32 scan
    np.testing.assert_allclose(li, me[f"{name}/lufs_inst"], rtol=0, atol=LU_TOL)
    tp = e.true_peak(frames)
    np.testing.assert_allclose(tp, me[f"{name}/tp"], rtol=0, atol=TP_TOL_DB)
    # record how close the float32 scan IIR actually is (well inside the 0.1 LU bar)
    assert np.max(np.abs(li - me[f"{name}/lufs_inst"])) < 0.01
    _, li64 = e.weighting(frames, "K", weighted=False)  # omega_weighting: scipy's float64 filtfilt
    assert np.max(np.abs(li64 - me[f"{name}/lufs_inst"])) < 1e-4


DC_SEQS = ["dc09_n1e4", "dc05_n1e3", "dcm07_n3e4", "dc03_sine", "dc09_sine1e3", "dc_step", "hann_dc05"]


@pytest.fixture(scope="module")
def mdc():
    return load_golden("meters_dc")


@pytest.mark.parametrize("name", DC_SEQS)
def test_meter_dc_offset_batch_path(mdc, name):
    """DC-biased 16384-sample frames (capture passes raw samples, capture.py:571-574) through the
    cfg2 batch launch (float32 K-weighting scan, true peak, meter aggregates) and the standalone
    float32 K-weighting kernel, against the reference's own calculate_lufs on the same frames
    (tests/golden/meters_dc.npz). A float32 direct-form filtfilt is ~0.1 LU off at 0.9 DC + 1e-4
    noise -- this scan was 6.09 LU off on dc09_n1e4, 0.91 on dcm07_n3e4 and 2.28 on dc_step (MI355X,
    round 4) before it filtered x - mean(x) (K(x) = K(x - c) exactly: both sections are high-passes
    with odd extension and lfilter_zi initial states); now <= 0.003 LU on the constant offsets. The
    Hann-windowed offset is not a constant and keeps 0.015 LU (0.044 before). Bars: 0.01 LU for the
    constant offsets, 0.03 for the Hann form (the north star's is 0.1)."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS, Resolution
    fr = S.dc_meter_frames()[name]
    n = len(fr)
    eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=1)
    out = eng.process_frames(torch.from_numpy(fr).cuda(), n, 16384, 16384, meters=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    bar = 0.03 if name.startswith("hann") else 0.01
    li_err = np.abs(out["lufs_inst"] - mdc[f"{name}/lufs_inst"])
    assert li_err.max() < bar, li_err
    assert np.abs(out["true_peak_db"] - mdc[f"{name}/tp"]).max() < TP_TOL_DB
    agg = mdc[f"{name}/agg"]
    assert np.abs(out["meters"][:, :4] - agg[:, :4]).max() < bar
    assert np.abs(out["meters"][:, 4] - agg[:, 4]).max() < TP_TOL_DB
    e = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)
    _, li = e.k_weighting_scan(fr, weighted=False)  # kweight_kernel: the same scan standalone
    assert np.abs(li - mdc[f"{name}/lufs_inst"]).max() < bar
    _, li64 = e.k_weighting(fr, weighted=False)  # omega_weighting: scipy's float64 cascade
    assert np.abs(li64 - mdc[f"{name}/lufs_inst"]).max() < 1e-4


def test_meter_dc_offset_facade_float64(mdc):
    """The app's call: float64 Hann-windowed frames into calculate_lufs / calculate_true_peak
    (omega4_main.py:1082). Values against the reference's, and the true peak's type follows the input
    like scipy's resample (professional_meters.py:289-299): float64 here, float32 for float32 frames."""
    from omega_gpu.professional_meters import ProfessionalMetering
    fr64 = S.dc_meter_frames()["dc05_n1e3"].astype(np.float64) * np.hanning(16384)
    pm = ProfessionalMetering(FS)
    agg = mdc["hann64_dc05/agg"]
    for f, x in enumerate(fr64):
        d = pm.calculate_lufs(x)
        got = np.array([d[k] for k in ("momentary", "short_term", "integrated", "range", "true_peak")])
        assert np.abs(got[:4] - agg[f, :4]).max() < 0.01, (f, got, agg[f])
        assert abs(got[4] - agg[f, 4]) < TP_TOL_DB
        assert type(d["true_peak"]) is np.float64 and type(d["integrated"]) is np.float64
    assert str(mdc["hann64_dc05/tp_dtype"]) == "float64" and str(mdc["dc09_n1e4/tp_dtype"]) == "float32"
    assert type(pm.calculate_true_peak(fr64[0])) is np.float64
    assert type(pm.calculate_true_peak(fr64[0].astype(np.float32))) is np.float32
    assert type(pm.calculate_true_peak(np.zeros(2048))) is float


def test_meter_long_window_batch(me):
    """3700 frames: the 3600-deep integrated window evicts; batched form on the device."""
    from omega_gpu.professional_meters import ProfessionalMetering
    pm = ProfessionalMetering(FS)
    out = pm.calculate_lufs_batch(S.level_steps(3700, 512, seed=9))
    g = me["long/agg"]
    assert np.max(np.abs(out[:, :4] - g[:, :4])) < LU_TOL
    assert np.max(np.abs(out[:, 4] - g[:, 4])) < TP_TOL_DB


def test_meter_aggregates_exact_on_injected_values(me):
    """A9 in isolation: with the oracle's instantaneous values (rounded to float32, as the device
    stores them) the aggregates -- means, gated mean, numpy-'linear' percentiles, peak hold -- match a
    float64 restatement to 1e-9, across batch boundaries (state carried between calls)."""
    from omega_gpu import Engine, Resolution
    li = me["long/lufs_inst"].astype(np.float32)
    tp = me["long/tp"].astype(np.float32)
    e = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)
    outs = [e.meter_update(li[a:b], tp[a:b], b - a) for a, b in ((0, 1), (1, 700), (700, 3650), (3650, 3700))]
    dev = np.concatenate(outs)
    st = R.MeterState(FS)
    ref = np.array([[v for v in st.update(np.ones(1), float(li[f]), float(tp[f])).values()] for f in range(3700)])
    np.testing.assert_allclose(dev, ref, rtol=0, atol=1e-9)


def test_meter_aggregates_random_batches():
    """Randomised stream: gated/ungated mixtures, silent stretches (no gated value in the window),
    repeated values, and batch sizes on both sides of the rank-sort / bitonic switch (1024) and the
    per-launch chunk (2048); exact against the float64 restatement."""
    from omega_gpu import Engine, Resolution
    rng = np.random.default_rng(5)
    n = 12000
    li = rng.uniform(-90, -5, n).astype(np.float32)
    li[3000:7000] = -95.0                        # a silent stretch: the window empties of gated values
    li[8000:8400] = np.float32(-23.0)            # ties
    tp = rng.uniform(-40, 0, n).astype(np.float32)
    e = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)
    cuts = np.cumsum([1, 17, 256, 1023, 1024, 1025, 2048, 2049, 3000, 5])
    cuts = [0] + [int(c) for c in cuts if c < n] + [n]
    dev = np.concatenate([e.meter_update(li[a:b], tp[a:b], b - a) for a, b in zip(cuts[:-1], cuts[1:])])
    st = R.MeterState(FS)
    ref = np.array([[v for v in st.update(np.ones(1), float(li[f]), float(tp[f])).values()] for f in range(n)])
    np.testing.assert_allclose(dev, ref, rtol=0, atol=1e-9)


def test_batched_frames_match_facade(me):
    """The fused batch path (process_frames with meters) equals frame-by-frame calculate_lufs."""
    from omega_gpu import Engine, Resolution
    frames = me["sine2048/x"]
    e = Engine([Resolution((20, 200), 2048, 512, 1.5)], FS, 20000, 64, n_channels=1)
    out = e.process_frames(frames.ravel(), len(frames), 2048, 2048, combined=False, meters=True)
    g = me["sine2048/agg"]
    assert np.max(np.abs(out["meters"][:, :4] - g[:, :4])) < LU_TOL
    assert np.max(np.abs(out["meters"][:, 4] - g[:, 4])) < TP_TOL_DB


def test_calculate_lufs_fused_equals_three_calls():
    """omega_calculate_lufs (weighting + true peak + aggregates, one host round trip) gives exactly what
    omega_weighting, omega_true_peak_os and omega_meter_update give one after the other, over a run
    of stereo frames in every weighting mode."""
    from omega_gpu import Engine, Resolution
    rng = np.random.default_rng(11)
    x = (0.2 * rng.standard_normal((40 * 2, 2048))).astype(np.float32)
    for mode in ("K", "A", "C", "Z"):
        kw = dict(sample_rate=FS, max_freq=20000, target_bins=2, frame_size=512, n_channels=2)
        e1 = Engine([Resolution((20, 20000), 512, 256, 1.0)], **kw)
        e2 = Engine([Resolution((20, 20000), 512, 256, 1.0)], **kw)
        li, tp, met = e1.calculate_lufs(x, mode)
        _, li2 = e2.weighting(x, mode, weighted=False)
        tp2 = e2.true_peak(x)
        met2 = e2.meter_update(li2, tp2, 40)
        np.testing.assert_array_equal(li, li2)
        np.testing.assert_array_equal(tp, tp2)
        np.testing.assert_array_equal(met, met2)


def test_calculate_lufs_interleaved_with_batches():
    """omega_calculate_lufs joins the side stream by a device counter (its true peaks count in, the
    first meter prep polls it) while only its own true peaks went there, and by an event once a batch's
    meter prep did: calls interleaved with process_frames batches on one context, and repeated calls in
    a row, give bitwise what the same sequence gives with the host synchronised after every call."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    xb = torch.from_numpy(S.cfg2_batch(32, seed_l=21, seed_r=22)).cuda()
    rng = np.random.default_rng(23)
    xs = (0.2 * rng.standard_normal((9, 2, 2048))).astype(np.float32)
    res = []
    for sync in (False, True):
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        outs = []
        for k in range(9):
            if k in (0, 5):
                o = eng.process_frames(xb[16 * (k // 5):16 * (k // 5) + 16], 16, 2 * 16384, 16384, meters=True)
                if sync:
                    eng.synchronize()
                    torch.cuda.synchronize()
                outs.append(o["meters"])
            li, tp, met = eng.calculate_lufs(xs[k], "K")
            outs.extend([li, tp, met])
            if sync:
                eng.synchronize()
        eng.synchronize()
        torch.cuda.synchronize()
        res.append([o.cpu().numpy() if hasattr(o, "cpu") else o for o in outs])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_calculate_lufs_refused_calls_leave_the_next_call_right():
    """A batch whose meter prep went to the side stream, then two omega_calculate_lufs calls the library
    refuses (oversampling 3; frames of 9 samples in mode K: scipy's padlen), then three good ones on
    2048-sample frames: the refusals keep their error class and text, change no meter state and leave the
    side stream unjoined-but-marked, so every output equals, bitwise, a context that ran the batch and the
    good calls alone with the host synchronised after each. What this cannot do: where a refused call
    wrongly marked the side stream joined, the next call's aggregates only raced the batch's prep, and this
    test does not reliably lose that race. The rule itself -- only a join clears the mark, a call that ends
    before its join leaves it -- is pinned on the CPU (tests/test_meter_sync.py)."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    from omega_gpu._lib import OmegaError, UnsupportedError
    xb = torch.from_numpy(S.cfg2_batch(16, seed_l=31, seed_r=32)).cuda()
    rng = np.random.default_rng(33)
    xs = (0.2 * rng.standard_normal((3, 2, 2048))).astype(np.float32)
    res = []
    for refused in (True, False):
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        o = eng.process_frames(xb, 16, 2 * 16384, 16384, meters=True)
        outs = [o[k] for k in sorted(o)]
        if refused:
            with pytest.raises(UnsupportedError) as err:
                eng.calculate_lufs(xs[0], "K", oversampling=3)
            assert str(err.value) == "libomega error -4: true peak: oversampling 3 unsupported (1, 2, 4)"
            with pytest.raises(OmegaError) as err:
                eng.calculate_lufs(xs[0][:, :9], "K")
            assert type(err.value) is OmegaError
            assert str(err.value) == ("libomega error -1: weighting: the length of the input (9) must be greater "
                                      "than padlen (9)")
        else:
            eng.synchronize()
            torch.cuda.synchronize()
        for k in range(3):
            outs.extend(eng.calculate_lufs(xs[k], "K"))
            if not refused:
                eng.synchronize()
        eng.synchronize()
        torch.cuda.synchronize()
        res.append([v.cpu().numpy() if hasattr(v, "cpu") else v for v in outs])
    assert len(res[0]) == len(res[1]) == 4 + 9
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_calculate_lufs_grows_the_any_length_scratch():
    """Frames of 6860 = 4 * 5 * 7^3 samples, past the 6826-sample limit of the LDS transform: the true peak
    of omega_calculate_lufs, on the side stream, runs through the any-length transform's global scratch,
    which the second call (4 stereo frames after 1) replaces by a larger one. Both calls give bitwise what
    omega_weighting, omega_true_peak_os and omega_meter_update give on a second context."""
    from omega_gpu import Engine, Resolution
    rng = np.random.default_rng(41)
    kw = dict(sample_rate=FS, max_freq=20000, target_bins=2, frame_size=512, n_channels=2)
    e1 = Engine([Resolution((20, 20000), 512, 256, 1.0)], **kw)
    e2 = Engine([Resolution((20, 20000), 512, 256, 1.0)], **kw)
    for n_frames in (1, 4):
        x = (0.2 * rng.standard_normal((n_frames * 2, 6860))).astype(np.float32)
        li, tp, met = e1.calculate_lufs(x, "K")
        _, li2 = e2.weighting(x, "K", weighted=False)
        tp2 = e2.true_peak(x)
        met2 = e2.meter_update(li2, tp2, n_frames)
        np.testing.assert_array_equal(li, li2)
        np.testing.assert_array_equal(tp, tp2)
        np.testing.assert_array_equal(met, met2)


def test_meter_too_short_keeps_state():
    """A frame of 9 samples or fewer (scipy's filtfilt raises: padlen 9) is logged and the meters keep
    their state; 480 samples (not a power of two) is metered like the reference."""
    from omega_gpu.professional_meters import ProfessionalMetering
    pm = ProfessionalMetering(FS)
    before = dict(pm.calculate_lufs(S.sine(1000, 0.1, 2048)))
    after = pm.calculate_lufs(S.sine(1000, 0.1, 9))
    assert after == before
    assert pm.calculate_lufs(np.zeros(0, np.float32)) is pm.current_lufs
    st = R.MeterState(FS)
    st.update(S.sine(1000, 0.1, 2048))
    ref = st.update(S.sine(1000, 0.1, 480))
    got = pm.calculate_lufs(S.sine(1000, 0.1, 480))
    for k in ("momentary", "short_term", "integrated", "range"):
        assert abs(got[k] - ref[k]) < 1e-3, k
    assert abs(got["true_peak"] - ref["true_peak"]) < TP_TOL_DB


@pytest.mark.parametrize("name", ["hist4800", "peaks4800", "square480", "noise1000", "prime1021", "smooth4410",
                                  "long9600", "tiny10"])
def test_meters_any_length_golden(name):
    """Frames of any length (the reference's 100 ms chunks of test_enhanced_meters.py:82-135, odd,
    prime and 7-smooth lengths, 9600 samples through the global-scratch transform): LUFS_inst from the
    float64 weighting cascade, the true peak at 4x / 2x / 1x from the mixed-radix transform, and the
    aggregate dicts frame by frame, against the reference's outputs."""
    from omega_gpu import Engine, Resolution
    from omega_gpu.professional_meters import ProfessionalMetering
    g = load_golden("meters_any")
    fr = g[f"{name}/x"]
    e = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512)
    _, li = e.weighting(fr, "K", weighted=False)
    assert np.max(np.abs(li - g[f"{name}/lufs_inst"])) < 1e-4
    for o, key in ((4, "tp"), (2, "tp2"), (1, "tp1")):
        np.testing.assert_allclose(e.true_peak(fr, o), g[f"{name}/{key}"], rtol=0, atol=TP_TOL_DB, err_msg=f"{o}x")
    pm = ProfessionalMetering(FS)
    agg = g[f"{name}/agg"]
    for f, x in enumerate(fr):
        d = pm.calculate_lufs(x)
        got = np.array([d[k] for k in ("momentary", "short_term", "integrated", "range", "true_peak")])
        assert np.all(np.abs(got[:4] - agg[f, :4]) < 1e-3), (f, got, agg[f])
        assert abs(got[4] - agg[f, 4]) < TP_TOL_DB
    y = pm.apply_k_weighting(fr[0])
    assert normwise(y, g[f"{name}/kw0"]) < 1e-6


@pytest.mark.parametrize("m", [1, 2, 3, 5, 7, 100, 1000, 1021, 1024, 8192, 16384])
def test_true_peak_oversampling(m):
    """calculate_true_peak(x, oversampling) for 1, 2 and 4 (phase subsets of the polyphase transform)
    against scipy's resample (the oracle), at every frame length omega_true_peak_os accepts (m >= 1:
    the power-of-two kernels and the mixed-radix path down to one sample); an unsupported factor is
    logged and the previous value returned. TP_TOL_DB is the north-star bar only: the float32-accuracy
    comparison of every path, phase by phase, is tests/test_true_peak_phases.py (eps32 log2(4N) at most)."""
    from omega_gpu.professional_meters import ProfessionalMetering
    pm = ProfessionalMetering(FS)
    x = S.sine(997, 0.4, m) + S.noise(31, m, 0.05)
    for o in (4, 2, 1):
        got = pm.calculate_true_peak(x, o)
        assert abs(got - R.true_peak(x, o)) < TP_TOL_DB, (m, o)
    tp4, tp2, tp1 = (float(pm.calculate_true_peak(x, o)) for o in (4, 2, 1))
    assert tp4 >= tp2 - 1e-4 and tp2 >= tp1 - 1e-4  # more phases never lower the peak
    prev = pm.calculate_true_peak(x, 4)
    assert pm.calculate_true_peak(x, 3) == prev


@pytest.mark.parametrize("fs", [48000, 44100])
@pytest.mark.parametrize("mode", ["A", "C"])
def test_ac_weighting_golden(fs, mode):
    """apply_a_weighting / apply_c_weighting (professional_meters.py:155-218) on the device: scipy's
    float64 filtfilt cascade (first-order sections with padlen 6) as chunked scans (weight64.hip),
    against the reference's outputs: float32 output rounding only."""
    from omega_gpu.professional_meters import ProfessionalMetering
    g = load_golden("weighting_ac")
    pm = ProfessionalMetering(fs)
    for name in ("sine2048", "comp4800", "hann2048_f64", "low50_4096", "noise16384", "quiet1024"):
        x = g[f"{fs}/{name}/x"]
        y = pm.apply_a_weighting(x) if mode == "A" else pm.apply_c_weighting(x)
        ref = g[f"{fs}/{name}/{mode}"]
        assert y.dtype == np.float64 and y.shape == ref.shape
        if not ref.any():
            assert not y.any(), name  # RMS gate
            continue
        assert normwise(y, ref) < 1e-6, (name, normwise(y, ref))
        lu = 10 * np.log10(np.mean(y ** 2)) - 10 * np.log10(np.mean(ref ** 2))
        assert abs(lu) < 1e-4, (name, lu)
    pm.weighting_mode = mode
    x = g[f"{fs}/sine2048/x"]
    np.testing.assert_array_equal(pm.apply_weighting(x), pm.apply_a_weighting(x) if mode == "A" else pm.apply_c_weighting(x))


@pytest.mark.parametrize("mode", ["A", "C"])
def test_ac_weighting_lufs_sequence(mode):
    """calculate_lufs with weighting_mode A / C (the panel's mode switch, professional_meters.py:552)
    against the reference's aggregate dicts, frame by frame and batched."""
    from omega_gpu.professional_meters import ProfessionalMetering
    g = load_golden("weighting_ac")
    agg = g[f"seq/{mode}/agg"]
    pm = ProfessionalMetering(FS)
    pm.weighting_mode = mode
    for f, x in enumerate(g["seq/x"]):
        d = pm.calculate_lufs(x)
        got = np.array([d[k] for k in ("momentary", "short_term", "integrated", "range", "true_peak")])
        assert np.all(np.abs(got[:4] - agg[f, :4]) < LU_TOL), (f, got, agg[f])
        assert abs(got[4] - agg[f, 4]) < TP_TOL_DB
    pm2 = ProfessionalMetering(FS)
    pm2.weighting_mode = mode
    out = pm2.calculate_lufs_batch(g["seq/x"])
    assert np.max(np.abs(out[:, :4] - agg[:, :4])) < LU_TOL


def test_bands_golden(golden):
    from omega_gpu.bands import PipelineBands, PrecomputedFrequencyMapper
    g = golden("bands")
    mags = g["mags8192"]
    for nb, fft in ((512, 8192), (768, 4096)):
        pb = PipelineBands(FS, nb, fft)
        np.testing.assert_array_equal(pb.starts, g[f"pipe{nb}_{fft}/starts"])
        np.testing.assert_array_equal(pb.ends, g[f"pipe{nb}_{fft}/ends"])
        src = mags if fft == 8192 else mags[:, : fft // 2 + 1]
        out = np.stack([pb.map_to_bands(m, apply_smoothing=False) for m in src])
        np.testing.assert_allclose(out, g[f"pipe{nb}_{fft}/out"], rtol=1e-6)
        sm = np.stack([pb.map_to_bands(m, apply_smoothing=True) for m in src])
        np.testing.assert_allclose(sm, g[f"pipe{nb}_{fft}/smooth"], rtol=1e-6)
    for fft, nb in ((2048, 512), (8192, 512)):
        fm = PrecomputedFrequencyMapper(FS, fft, nb)
        np.testing.assert_array_equal(np.array(fm.band_indices), g[f"mel{fft}_{nb}/bands"])
        spec = g[f"mel{fft}_{nb}/spec"]
        np.testing.assert_allclose(np.stack([fm.map_spectrum_to_bars(s, True) for s in spec]),
                                   g[f"mel{fft}_{nb}/out_comp"], rtol=1e-5)
        np.testing.assert_allclose(np.stack([fm.map_spectrum_to_bars(s, False) for s in spec]),
                                   g[f"mel{fft}_{nb}/out_raw"], rtol=1e-5)
        np.testing.assert_allclose(np.stack([fm.map_spectrum_to_bars(s[:512], False) for s in spec]),
                                   g[f"mel{fft}_{nb}/out_512in"], rtol=1e-5)


def test_chroma_golden(golden):
    from omega_gpu.chromagram import ChromagramAnalyzer
    g = golden("chroma")
    ca = ChromagramAnalyzer(FS)
    out = np.stack([ca.compute_chromagram(m, g["freqs"]) for m in g["mags"]])
    np.testing.assert_allclose(out, g["out"], rtol=1e-6, atol=1e-9)
    a = ChromagramAnalyzer(FS).compute_chromagram(g["a440_mag"], g["freqs"])
    assert int(np.argmax(a)) == 9
    np.testing.assert_allclose(a, g["a440_out"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("genre", ["metal", "rock", "jazz"])
def test_chroma_genre_golden(golden, genre):
    """Metal / rock tuning offsets (drop D, E, Eb; the 30-deep mode) and the jazz blend against the
    reference's own sequences; per frame and batched."""
    from omega_gpu.chromagram import ChromagramAnalyzer
    g = golden("chroma_genre")
    ca = ChromagramAnalyzer(FS)
    ca.current_genre = genre
    out, offs = [], []
    for m in g["mags"]:
        out.append(ca.compute_chromagram(m, g["freqs"]))
        offs.append(ca.transposition_offset)
    np.testing.assert_array_equal(offs, g[f"{genre}/offset"])
    np.testing.assert_allclose(np.stack(out), g[f"{genre}/out"], rtol=1e-6, atol=1e-9)
    cb = ChromagramAnalyzer(FS)
    cb.current_genre = genre
    np.testing.assert_allclose(cb.compute_chromagram_batch(g["mags"], g["freqs"]), g[f"{genre}/out"],
                               rtol=1e-6, atol=1e-9)


def test_gpu_accelerated_fft_golden(golden):
    """GPUAcceleratedFFT facade: compute_fft per window and input dtype (float32 device transform vs
    the reference's CPU branch, 1e-4 normwise), its first-100-bytes cache, the multi-resolution
    dict with a zero-padded size, process_fft_batch on device tensors, lengths of any factorization. The
    1e-4 is the north-star bar only: the float32-accuracy comparison, bin by bin on designed signals, is
    tests/test_pow2_rfft_bins.py (powers of two 512..16384) and tests/test_any_rfft.py (other lengths)."""
    import torch
    from omega_gpu.gpu_accelerated_fft import GPUAcceleratedFFT
    g = golden("gpufft")
    ga = GPUAcceleratedFFT()
    for name, w in (("noise_4096_hann", "hann"), ("comp_f64_2048_hamming", "hamming"),
                    ("triad_8192_blackman", "blackman"), ("sine_16384_hann", "hann")):
        mag, cp = ga.compute_fft(g[f"fft/{name}/x"], w)
        assert normwise(mag, g[f"fft/{name}/mag"]) < SPEC_TOL, name
        assert np.abs(cp - g[f"fft/{name}/complex"]).max() / np.abs(g[f"fft/{name}/complex"]).max() < SPEC_TOL
    gc = GPUAcceleratedFFT()
    ma = gc.compute_fft(g["cache/a"], "hann")[0]
    mb = gc.compute_fft(g["cache/b"], "hann")[0]
    assert mb is ma  # the reference's prefix cache: the same cached spectrum
    assert normwise(mb, g["cache/mag_b"]) < SPEC_TOL
    res = GPUAcceleratedFFT().compute_multi_resolution_fft(g["multi/x"], {"bass": 8192, "mid": 4096, "high": 1024})
    for k in ("bass", "mid", "high"):
        assert normwise(res[k]["magnitude"], g[f"multi/{k}/magnitude"]) < SPEC_TOL, k
        np.testing.assert_array_equal(res[k]["freqs"], g[f"multi/{k}/freqs"])
    inp, _ = ga.prepare_batch_arrays(3, 4096)
    x = np.stack([S.noise(s, 4096, 0.2) for s in (1, 2, 3)])
    inp.copy_(torch.from_numpy(x))
    out = ga.process_fft_batch(inp, "hamming")
    assert out.is_cuda and out.dtype == torch.complex64 and out.shape == (3, 2049)
    ref = np.stack([R.gpu_fft(r, "hamming")[1] for r in x])
    assert np.abs(out.cpu().numpy() - ref).max() / np.abs(ref).max() < SPEC_TOL
    # lengths off the power-of-two kernels: the mixed-radix transform (anyfft.hip), 7-smooth and prime
    for n in (3000, 1021):
        xb = np.stack([S.noise(s, n, 0.2) for s in (4, 5)])
        out = ga.process_fft_batch(torch.from_numpy(xb).cuda(), "hann")
        ref = np.stack([R.gpu_fft(r, "hann")[1] for r in xb])
        assert out.shape == (2, n // 2 + 1) and np.abs(out.cpu().numpy() - ref).max() / np.abs(ref).max() < SPEC_TOL
        mag, _ = ga.compute_fft(xb[0], "blackman")
        assert normwise(mag, R.gpu_fft(xb[0], "blackman")[0]) < SPEC_TOL


def test_batched_fft_golden(golden):
    from omega_gpu.batched_fft_processor import BatchedFFTProcessor
    g = golden("batched")
    bp = BatchedFFTProcessor()
    cases = (("app_f64_2048_hann", 2048, "hann"), ("f32_4096_blackman", 4096, "blackman"),
             ("pad_1000_1024_hamming", 1024, "hamming"), ("trim_20000_16384_hann", 16384, "hann"))
    ids = {name: bp.prepare_batch(name, g[f"{name}/x"], n, w) for name, n, w in cases}
    assert bp.process_batch() == 4
    res = bp.distribute_results()
    for name, n, w in cases:
        r = res[ids[name]]
        assert normwise(r["magnitude"], g[f"{name}/mag"]) < SPEC_TOL
        gc = g[f"{name}/complex"]
        assert np.max(np.abs(r["complex"] - gc)) / np.max(np.abs(gc)) < SPEC_TOL


# ---- BASELINE cfg2 at full size: size-independent properties + sampled oracle parity ----

@pytest.fixture(scope="module")
def cfg2():
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    x = S.cfg2_batch(256)
    eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    xd = torch.from_numpy(x).cuda()
    out = eng.process_frames(xd, 256, 2 * 16384, 16384, meters=True)
    torch.cuda.synchronize()
    return x, eng, xd, {k: v.cpu().numpy() for k, v in out.items()}


def test_cfg2_all_frames_match_oracle(cfg2):
    """Every one of the 512 channel-frames of the headline batch against the oracle (~2 s of numpy)."""
    x, _, _, out = cfg2
    worst = np.zeros(3)
    for f in range(256):
        for c in range(2):
            res, comb, li, tp = R.full_frame(x[f, c])
            cf = f * 2 + c
            e = (normwise(out["combined"][cf], comb), abs(out["lufs_inst"][cf] - li), abs(out["true_peak_db"][cf] - tp))
            assert e[0] < SPEC_TOL and e[1] < LU_TOL and e[2] < TP_TOL_DB, (f, c, e)
            worst = np.maximum(worst, e)
    # the measured margins (round 4: spectra ~4e-7 normwise, LUFS ~1e-4 LU, TP ~1e-5 dB)
    assert worst[0] < 1e-5 and worst[1] < 0.01 and worst[2] < 1e-3, worst


def test_cfg2_combine_only_matches_magnitude_path(cfg2):
    """Without magnitude outputs the batch's resolutions combine straight from the packed spectra (the
    16384-point one forms only its lowest and highest 256 frequencies, RegFFT::run_low); with them, every
    bin's magnitude is formed first. Both must give the same combined spectrum on all 512 channel-frames
    (float32 rounding apart: the two paths take the untangle twiddles from different forms)."""
    import torch
    x, eng, xd, out = cfg2
    eng.reset_meters()
    full = eng.process_frames(xd, 256, 2 * 16384, 16384, mags=True)
    torch.cuda.synchronize()
    fc = full["combined"].cpu().numpy()
    err = np.abs(fc - out["combined"]).max(axis=1) / np.abs(fc).max(axis=1)
    assert err.max() < 1e-5, err.max()


def test_cfg2_properties(cfg2):
    import torch
    x, eng, xd, out = cfg2
    assert np.isfinite(out["combined"]).all() and (out["combined"] >= 0).all()
    peak_db = 20 * np.log10(np.abs(x).max(axis=2)).reshape(-1)
    assert (out["true_peak_db"] >= peak_db - 1e-4).all()  # true peak >= sample peak
    # linearity: 2x input -> 2x spectrum, +6.02 dB LUFS and true peak
    eng.reset_meters()
    o2 = eng.process_frames(xd * 2, 256, 2 * 16384, 16384)
    torch.cuda.synchronize()
    np.testing.assert_allclose(o2["combined"].cpu().numpy(), 2 * out["combined"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o2["lufs_inst"].cpu().numpy() - out["lufs_inst"], 20 * np.log10(2), atol=1e-3)
    np.testing.assert_allclose(o2["true_peak_db"].cpu().numpy() - out["true_peak_db"], 20 * np.log10(2), atol=1e-3)
    # determinism: the same launch twice is bitwise identical
    o3 = eng.process_frames(xd * 2, 256, 2 * 16384, 16384)
    torch.cuda.synchronize()
    for k in ("combined", "lufs_inst", "true_peak_db"):
        assert torch.equal(o2[k], o3[k])


def test_cfg2_meter_state_matches_oracle_sequence(cfg2):
    """meters[f, c] after the batch equal 256 sequential calculate_lufs calls per channel."""
    x, _, _, out = cfg2
    li = out["lufs_inst"].reshape(256, 2)
    tp = out["true_peak_db"].reshape(256, 2)
    for c in (0, 1):
        st = R.MeterState(FS)
        ref = np.array([list(st.update(np.ones(1), float(li[f, c]), float(tp[f, c])).values()) for f in range(256)])
        np.testing.assert_allclose(out["meters"].reshape(256, 2, 5)[:, c], ref, rtol=0, atol=1e-9)


def test_cfg4_shard_packed_outputs_match_oracle():
    """BASELINE cfg4's per-GPU shard (4096 stereo frames x 16384 = 8192 channel-frames, two meter
    chunks per channel) through bench.py's own zero-copy packed output block: sampled frames against
    the oracle (first/last, both sides of the meter-chunk boundary), the meter aggregates of all 4096
    frames per channel against the oracle's sequential calculate_lufs calls on the device's
    instantaneous values, and full-size properties (finite, TP >= sample peak, bitwise repeatable)."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    from omega_gpu import dist as D
    F = 4096
    x = S.cfg2_batch(F, seed_l=6, seed_r=7)  # rank 3's seeds
    xd = torch.from_numpy(x).cuda()
    eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    lay = D.PackedLayout(2 * F, 512)
    bufs = [lay.alloc("cuda"), lay.alloc("cuda")]
    eng.process_frames(xd, F, 2 * 16384, 16384, meters=True, out=lay.views(bufs[0]))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in lay.views(bufs[0]).items()}
    # 256 frames x 2 channels against the oracle: the first and last 64 frames and 128 across the
    # boundary of the two meter chunks (kMeterChunk = 2048 frames per channel)
    for f in list(range(64)) + list(range(1984, 2112)) + list(range(4032, 4096)):
        for c in (0, 1):
            _, comb, li, tp = R.full_frame(x[f, c])
            cf = f * 2 + c
            assert normwise(out["combined"][cf], comb) < SPEC_TOL, (f, c)
            assert abs(out["lufs_inst"][cf] - li) < LU_TOL, (f, c)
            assert abs(out["true_peak_db"][cf] - tp) < TP_TOL_DB, (f, c)
    assert np.isfinite(out["combined"]).all() and np.isfinite(out["meters"]).all()
    peak_db = 20 * np.log10(np.abs(x).max(axis=2)).reshape(-1)
    assert (out["true_peak_db"] >= peak_db - 1e-4).all()
    li = out["lufs_inst"].reshape(F, 2)
    tp = out["true_peak_db"].reshape(F, 2)
    for c in (0, 1):
        st = R.MeterState(FS)
        ref = np.array([list(st.update(np.ones(1), float(li[f, c]), float(tp[f, c])).values()) for f in range(F)])
        np.testing.assert_allclose(out["meters"].reshape(F, 2, 5)[:, c], ref, rtol=0, atol=1e-9)
    # the same batch again into the other buffer (a fresh meter stream): bitwise identical
    eng.reset_meters()
    eng.process_frames(xd, F, 2 * 16384, 16384, meters=True, out=lay.views(bufs[1]))
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1])


def test_time_sharded_stream_meters_on_device():
    """SURVEY §8(e)'s time-sharded layout on the device: one stereo stream's frames split over three
    'ranks' (three contexts in this process; the all-gather replaced by handing the tails over), over
    two global batches, each rank loading the exchanged history (omega_gpu.dist.meter_time_shard:
    reset, the history through omega_meter_update, then its shard) -- bitwise equal to ONE context
    metering the whole stream. The LUFS / TP rows come from a cfg2-shaped batch launch."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS, Resolution
    from omega_gpu import dist as D
    rng = np.random.default_rng(21)
    n = 9000
    li = torch.from_numpy(rng.uniform(-85, -5, (n, 2)).astype(np.float32)).cuda()
    li[1200:1500] = -95.0
    tp = torch.from_numpy(rng.uniform(-40, 0, (n, 2)).astype(np.float32)).cuda()
    # plus real LUFS / TP rows of the batch launch at the front of the stream
    eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    o = eng.process_frames(torch.from_numpy(S.cfg2_batch(64)).cuda(), 64, 2 * 16384, 16384, combined=False)
    li[:64], tp[:64] = o["lufs_inst"].view(64, 2), o["true_peak_db"].view(64, 2)
    kw = dict(sample_rate=FS, max_freq=20000, target_bins=2, frame_size=512, n_channels=2)
    one = Engine([Resolution((20, 20000), 512, 256, 1.0)], **kw).meter_update(li, tp, n).view(n, 2, 5)
    world = 3
    ranks = [Engine([Resolution((20, 20000), 512, 256, 1.0)], **kw) for _ in range(world)]
    prev = (li[:0], tp[:0])
    for a0, b0 in ((0, 5000), (5000, n)):
        bl, bt = li[a0:b0], tp[a0:b0]
        blocks = [D.shard_range(b0 - a0, r, world) for r in range(world)]
        tails = [(bl[a:b][-D.LUFS_HIST:], bt[a:b][-D.TP_HIST:]) for a, b in blocks]
        for r, (a, b) in enumerate(blocks):
            hist = D.stream_history(prev[0], prev[1], tails, r)
            got = D.meter_time_shard(ranks[r], bl[a:b], bt[a:b], hist).view(-1, 2, 5)
            assert torch.equal(got, one[a0 + a:a0 + b]), (a0, r)
        prev = D.stream_history(prev[0], prev[1], tails, world)


def test_many_contexts_batch_meters():
    """Contexts created one after another in one process (each holds two streams; HIP deals streams out
    over 4 hardware queues per process): on every one of them the default batch path -- the batch kernel
    and the side stream's meter prep ordered by device counters, which needs the two on different queues
    (capi_core.cpp side_stream_check) -- returns without OMEGA_EHIP and bitwise the outputs of the first context,
    through the context's own stream and through torch's stream."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    x = torch.from_numpy(S.cfg2_batch(32)).cuda()
    engs, ref = [], None
    for k in range(6):
        e = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        engs.append(e)
        for _ in range(2):
            o = e.process_frames(x, 32, 2 * 16384, 16384, meters=True)
            e.synchronize()
        o = {k2: v.cpu() for k2, v in o.items()}
        if ref is None:
            ref = o
        for k2 in ref:
            assert torch.equal(o[k2], ref[k2]), (k, k2)
        # and a host-memory call (the context's own stream)
        h = e.process_frames(x.cpu().numpy(), 32, 2 * 16384, 16384, meters=True)
        assert np.array_equal(h["combined"], ref["combined"].numpy())


def test_side_stream_reprobed_with_busy_streams():
    """An RCCL-like neighbour: four more streams created after the context, each with a long-running
    kernel in flight (torch.cuda._sleep), then omega_check_queues re-probes the pair (capi_core.cpp
    side_stream_check) and in-call and pipelined batches with meters run beside them: no OMEGA_EHIP, and
    every output bitwise what the same sequence gives on a quiet context."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    x = torch.from_numpy(S.cfg2_batch(32)).cuda()

    def sequence(e):
        got = []
        for pipe in (False, True, False):
            e.set_meter_pipelining(pipe)
            for _ in range(2):
                o = e.process_frames(x, 32, 2 * 16384, 16384, meters=True)
                e.flush_meters()
                got.append({k: v.clone() for k, v in o.items()})
        e.synchronize()
        return [{k: v.cpu() for k, v in o.items()} for o in got]

    quiet = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    ref = sequence(quiet)
    quiet.close()
    e = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    streams = [torch.cuda.Stream() for _ in range(4)]
    for st in streams:
        with torch.cuda.stream(st):
            torch.cuda._sleep(20_000_000)  # ~10 ms each, in flight while the batches run
    independent = e.check_queues()
    got = sequence(e)
    torch.cuda.synchronize()
    assert isinstance(independent, bool)
    for a, b in zip(ref, got):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    # a switch back to an already-probed stream does not probe again, and the context keeps working
    with torch.cuda.stream(streams[0]):
        o = e.process_frames(x, 32, 2 * 16384, 16384, meters=False)
    torch.cuda.synchronize()
    assert torch.equal(o["combined"].cpu(), ref[0]["combined"])


def test_meter_load_history_longer_than_windows():
    """A context with shorter meter windows (integrated 600 frames, true peak 30) handed the time-shard
    exchange's full 3599 / 59-row history: omega_meter_load_history keeps the rows its windows hold, and
    the shard metered after it is bitwise what the replay of every row gives."""
    import torch
    from omega_gpu import Engine, Resolution
    from omega_gpu import dist as D
    rng = np.random.default_rng(11)
    hl = torch.from_numpy(rng.uniform(-90, -5, (3599, 2)).astype(np.float32)).cuda()
    ht = torch.from_numpy(rng.uniform(-40, 0, (59, 2)).astype(np.float32)).cuda()
    sl = torch.from_numpy(rng.uniform(-80, -5, (300, 2)).astype(np.float32)).cuda()
    st = torch.from_numpy(rng.uniform(-40, 0, (300, 2)).astype(np.float32)).cuda()
    kw = dict(sample_rate=FS, max_freq=20000, target_bins=2, frame_size=512, n_channels=2,
              meter_windows=(24, 180, 600, 30))
    a, b = (Engine([Resolution((20, 20000), 512, 256, 1.0)], **kw) for _ in range(2))
    got = D.meter_time_shard(a, sl, st, (hl, ht))
    b.reset_meters()
    rl, rt = D.history_frames(hl, ht)
    b.meter_update(rl.contiguous(), rt.contiguous(), rl.shape[0])
    ref = b.meter_update(sl, st, 300)
    assert torch.equal(got, ref)


def test_meter_load_history_refused_rows_leave_the_stream():
    """load_meter_history validates dtype and shape before it binds the stream: a refused history, given
    under another torch stream, leaves the context on the stream it had; an accepted one moves it."""
    import ctypes
    import torch
    from omega_gpu import _lib as L
    from omega_gpu import Engine, Resolution
    e = Engine([Resolution((20, 20000), 512, 256, 1.0)], FS, 20000, 2, frame_size=512, n_channels=2)
    stream_of = lambda: L.lib().omega_get_stream(e._ctx)  # noqa: E731
    rows = torch.full((8, 2), -20.0, device="cuda")
    e.load_meter_history(rows, rows)
    before = stream_of()
    side = torch.cuda.Stream()
    assert ctypes.c_void_p(side.cuda_stream).value != before
    with torch.cuda.stream(side):
        for bad in (rows[:, 0], rows.double(), torch.full((8, 3), -20.0, device="cuda")):
            with pytest.raises(ValueError, match="load_meter_history"):
                e.load_meter_history(bad, bad)
            assert stream_of() == before
        e.load_meter_history(rows, rows)
        assert stream_of() == ctypes.c_void_p(side.cuda_stream).value
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_l,n_t", [(0, 0), (1, 1), (40, 40), (100, 30), (3599, 59), (2500, 0)])
def test_meter_load_history_equals_replay(n_l, n_t):
    """omega_meter_load_history writes the meter state of a stream with the given LUFS_inst / true-peak
    history in one kernel; the shard metered after it is bitwise what the replay (reset, the history
    through omega_meter_update as pseudo-frames with -100 true peaks before the given ones) gives --
    gated and ungated values, a history shorter than the peak window, longer than the chunk."""
    import torch
    from omega_gpu import Engine, Resolution
    from omega_gpu import dist as D
    rng = np.random.default_rng(n_l + 7 * n_t)
    hl = torch.from_numpy(rng.uniform(-90, -5, (n_l, 2)).astype(np.float32)).cuda()
    ht = torch.from_numpy(rng.uniform(-40, 0, (n_t, 2)).astype(np.float32)).cuda()
    sl = torch.from_numpy(rng.uniform(-80, -5, (300, 2)).astype(np.float32)).cuda()
    st = torch.from_numpy(rng.uniform(-40, 0, (300, 2)).astype(np.float32)).cuda()
    kw = dict(sample_rate=FS, max_freq=20000, target_bins=2, frame_size=512, n_channels=2)
    a, b = (Engine([Resolution((20, 20000), 512, 256, 1.0)], **kw) for _ in range(2))
    a.load_meter_history(hl, ht)
    got = a.meter_update(sl, st, 300)
    b.reset_meters()
    rl, rt = D.history_frames(hl, ht)
    if n_l:
        b.meter_update(rl.contiguous(), rt.contiguous(), n_l)
    ref = b.meter_update(sl, st, 300)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("pipe", [False, True])
def test_many_contexts_default_layout(pipe):
    """The default layout's precondition (omega.h, omega_set_stream): the batch kernel and the meter
    prep on the context's side stream must be resident together. Six live contexts (12 streams of
    their own beside torch's, more than the 4 hardware queues a process has) each run the cfg2-shaped
    batch with meters in turn, three rounds: no ordering wait expires and every context gives the same
    outputs bitwise. With meter pipelining the side stream's stream wait follows the batch it waits
    for, so streams sharing a hardware queue serialise instead of blocking."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    x = torch.from_numpy(S.cfg2_batch(32)).cuda()
    engs = [Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2) for _ in range(6)]
    for e in engs:
        e.set_meter_pipelining(pipe)
    outs = [[] for _ in engs]
    for _ in range(3):
        for i, e in enumerate(engs):
            o = e.process_frames(x, 32, 2 * 16384, 16384, meters=True)
            outs[i].append(o)
    torch.cuda.synchronize()
    for e in engs:
        e.synchronize()  # raises OmegaError on an expired ordering wait
    for i in range(1, len(engs)):
        for r in range(3):
            for k in outs[0][r]:
                assert torch.equal(outs[0][r][k], outs[i][r][k]), (i, r, k)


def test_unsynchronised_calls_over_a_full_history():
    """Consecutive device calls with no host synchronisation between them, once the 3599-frame LUFS
    history is full (so every call's prep shifts it): the next call's meter prep may run while the
    previous batch's meter segment still reads the history -- the prep must not overwrite the slots the
    segment reads. Batches shorter and longer than the 30-frame short-term window, bitwise equal to the
    same calls each followed by a device synchronise, and equal to the oracle's sequential meters."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    rng = np.random.default_rng(33)
    n0 = 3700
    li0 = torch.from_numpy(rng.uniform(-60, -10, (n0, 2)).astype(np.float32)).cuda()
    tp0 = torch.from_numpy(rng.uniform(-30, 0, (n0, 2)).astype(np.float32)).cuda()
    sizes = [8, 16, 40, 4, 24, 12, 64, 8, 16]
    x = torch.from_numpy(S.cfg2_batch(sum(sizes), seed_l=8, seed_r=9)).cuda()
    res = []
    for sync in (False, True):
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        eng.meter_update(li0, tp0, n0)
        torch.cuda.synchronize()
        if not sync:
            torch.cuda._sleep(20_000_000)  # (~10 ms: every call below is queued before the first runs)
        outs, f0 = [], 0
        for n in sizes:
            outs.append(eng.process_frames(x[f0:f0 + n], n, 2 * 16384, 16384, combined=False, meters=True))
            f0 += n
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        eng.synchronize()
        res.append({k: torch.cat([o[k] for o in outs]).cpu().numpy() for k in outs[0]})
    for k in res[0]:
        np.testing.assert_array_equal(res[0][k], res[1][k], err_msg=k)
    n = sum(sizes)
    li = res[0]["lufs_inst"].reshape(n, 2)
    tp = res[0]["true_peak_db"].reshape(n, 2)
    h_li, h_tp = li0.cpu().numpy(), tp0.cpu().numpy()
    for c in (0, 1):
        st = R.MeterState(FS)
        for f in range(n0):
            st.update(np.ones(1), float(h_li[f, c]), float(h_tp[f, c]))
        ref = np.array([list(st.update(np.ones(1), float(li[f, c]), float(tp[f, c])).values()) for f in range(n)])
        np.testing.assert_allclose(res[0]["meters"].reshape(n, 2, 5)[:, c], ref, rtol=0, atol=1e-9)


def test_meter_pipelining_bitwise():
    """omega_set_meter_pipelining (omega.h): each batch call's meter aggregates are computed by the next
    call's launch (or a flush). Over a sequence that mixes pipelined calls of several sizes (one past
    the 2048-frame chunk: not pipelined, the pending segment runs first), a meter_update and a
    host-memory call (both flush), a stream switch and an explicit flush, all queued behind a sleep so
    that every kernel of the sequence is enqueued before the first runs: every output equals the
    non-pipelined context's bitwise."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    rng = np.random.default_rng(41)
    sizes = [64, 16, 256, 8, 2100, 32, 128, 4]
    x = torch.from_numpy(S.cfg2_batch(sum(sizes), seed_l=10, seed_r=11)).cuda()
    li_u = torch.from_numpy(rng.uniform(-50, -10, (40, 2)).astype(np.float32)).cuda()
    tp_u = torch.from_numpy(rng.uniform(-20, 0, (40, 2)).astype(np.float32)).cuda()
    side = torch.cuda.Stream()
    res = []
    for pipe in (False, True):
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        eng.set_meter_pipelining(pipe)
        torch.cuda.synchronize()
        torch.cuda._sleep(20_000_000)
        outs, f0 = [], 0
        for i, n in enumerate(sizes):
            xb = x[f0:f0 + n]
            f0 += n
            if i == 3:
                outs.append({"meters": eng.meter_update(li_u, tp_u, 40)})  # (flushes)
            if i == 5:  # host memory: synchronous, flushes first
                o = eng.process_frames(xb.cpu().numpy(), n, 2 * 16384, 16384, combined=False, meters=True)
                outs.append({k: torch.from_numpy(v) for k, v in o.items()})
                continue
            if i == 6:
                with torch.cuda.stream(side):
                    side.wait_stream(torch.cuda.current_stream())
                    outs.append(eng.process_frames(xb, n, 2 * 16384, 16384, meters=True))
                torch.cuda.current_stream().wait_stream(side)
                continue
            outs.append(eng.process_frames(xb, n, 2 * 16384, 16384, combined=(i % 2 == 0), meters=True))
            if i == 1:
                eng.flush_meters()
        eng.synchronize()  # (flushes the last call's meters)
        torch.cuda.synchronize()
        res.append([{k: v.cpu() for k, v in o.items()} for o in outs])
    for i, (a, b) in enumerate(zip(*res)):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)


def test_meter_pipelining_reset_and_destroy_flush():
    """A pending meter segment completes before omega_meter_reset replaces the state it reads, and at
    omega_destroy (the context's last call): the meters of both pending calls equal the unpipelined
    context's bitwise."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    x = torch.from_numpy(S.cfg2_batch(48, seed_l=12, seed_r=13)).cuda()
    res = []
    for pipe in (False, True):
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        eng.set_meter_pipelining(pipe)
        a = eng.process_frames(x[:32], 32, 2 * 16384, 16384, combined=False, meters=True)
        eng.reset_meters()  # (flushes a's segment first)
        b = eng.process_frames(x[32:], 16, 2 * 16384, 16384, combined=False, meters=True)
        eng.close()  # (flushes b's segment, then waits)
        torch.cuda.synchronize()
        res.append((a["meters"].cpu(), b["meters"].cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.isfinite(res[1][1]).all()


def test_meter_pipelining_reused_output_buffers():
    """with pipelining, call N's meter prep and deferred segment run during call N + 1. The
    caller's preallocated lufs_inst / true_peak_db / combined buffers, passed again to every call, are
    overwritten by call N + 1's batch while they run -- so they read the context's staging slots, not
    those buffers. Consecutive calls on one out dict (fresh meters per call, as omega.h asks), queued
    behind a sleep: meters bitwise equal to the unpipelined context's, and the shared buffers hold the
    last call's values."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    nb, n = 6, 32
    x = torch.from_numpy(S.cfg2_batch(nb * n, seed_l=14, seed_r=15)).cuda()
    x[n:2 * n] *= 0.25  # (batches of distinct loudness: a segment reading the wrong batch differs)
    res = []
    for pipe in (False, True):
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        eng.set_meter_pipelining(pipe)
        shared = {"combined": torch.empty(2 * n, 512, device="cuda"), "lufs_inst": torch.empty(2 * n, device="cuda"),
                  "true_peak_db": torch.empty(2 * n, device="cuda")}
        torch.cuda.synchronize()
        torch.cuda._sleep(20_000_000)
        mets = []
        for b in range(nb):
            o = dict(shared, meters=torch.empty(2 * n, 5, dtype=torch.float64, device="cuda"))
            mets.append(eng.process_frames(x[b * n:(b + 1) * n], n, 2 * 16384, 16384, meters=True, out=o)["meters"])
        eng.synchronize()
        torch.cuda.synchronize()
        res.append(([m.cpu() for m in mets], {k: v.cpu() for k, v in shared.items()}))
    for b in range(nb):
        assert torch.equal(res[0][0][b], res[1][0][b]), b
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_meter_pipelining_discarded_outputs():
    """the facade's default outputs of a pipelined call, all but meters discarded at once
    (``m = eng.process_frames(...)['meters']`` in a loop): torch's caching allocator hands the freed
    blocks to the next call, which writes them while the previous call's meters are still pending --
    harmless, since the pending work reads only the context's staging and writes the meters the caller
    keeps (Engine holds the pending call's outputs until its segment is enqueued). Bitwise equal to the
    unpipelined context."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    nb, n = 5, 16
    x = torch.from_numpy(S.cfg2_batch(nb * n, seed_l=16, seed_r=17)).cuda()
    x[2 * n:3 * n] *= 3.0
    res = []
    for pipe in (False, True):
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        eng.set_meter_pipelining(pipe)
        torch.cuda.synchronize()
        torch.cuda._sleep(20_000_000)
        mets = [eng.process_frames(x[b * n:(b + 1) * n], n, 2 * 16384, 16384, meters=True)["meters"]
                for b in range(nb)]
        eng.synchronize()
        torch.cuda.synchronize()
        res.append([m.cpu() for m in mets])
    for b in range(nb):
        assert torch.equal(res[0][b], res[1][b]), b


def test_stream_switch_keeps_meter_order():
    """Calls alternating between two torch streams (omega_set_stream on every call, Engine._bind_stream):
    the switch orders the new stream after the old one, so the meter state carried between calls is
    the same as on one stream -- bitwise, over consecutive 64-frame batches of one stereo stream."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    x = torch.from_numpy(S.cfg2_batch(256)).cuda()
    ref_e = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    alt_e = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ref, alt = [], []
    for b in range(4):
        xb = x[64 * b:64 * (b + 1)]
        ref.append(ref_e.process_frames(xb, 64, 2 * 16384, 16384, combined=False, meters=True)["meters"])
        with torch.cuda.stream(streams[b % 2]):
            alt.append(alt_e.process_frames(xb, 64, 2 * 16384, 16384, combined=False, meters=True)["meters"])
    torch.cuda.synchronize()
    for a, r in zip(alt, ref):
        assert torch.equal(a, r)


def test_meter_ordering_expiry_is_reported(monkeypatch):
    """The device-side ordering waits are bounded (meters.hip): when one expires the meters of that
    call may be stale, and the next omega_synchronize / omega_process_* call returns OMEGA_EHIP --
    once. OMEGA_POLL_LIMIT=1 (read at context creation) makes the meter prep give up after one poll,
    long before the K-weighting roles of a 4096-frame batch have counted in."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS, OmegaError
    monkeypatch.setenv("OMEGA_POLL_LIMIT", "1")
    eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    monkeypatch.delenv("OMEGA_POLL_LIMIT")
    xd = torch.from_numpy(S.cfg2_batch(2048)).cuda()
    seen = 0
    for _ in range(3):
        eng.process_frames(xd, 2048, 2 * 16384, 16384, meters=True)
        torch.cuda.synchronize()
        try:
            eng.synchronize()
        except OmegaError as e:
            assert "ordering wait expired" in str(e)
            seen += 1
            eng.synchronize()  # reported once: the flag is cleared
            break
    assert seen == 1
    # a host-memory call waits for its own results, so it reports its own expiry
    monkeypatch.setenv("OMEGA_POLL_LIMIT", "1")
    eng3 = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    monkeypatch.delenv("OMEGA_POLL_LIMIT")
    xh = S.cfg2_batch(2048)
    with pytest.raises(OmegaError, match="ordering wait expired"):
        eng3.process_frames(xh, 2048, 2 * 16384, 16384, meters=True)
    eng3.synchronize()  # (reported once)
    # a context with the default bound never reports it
    eng2 = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    eng2.process_frames(xd, 2048, 2 * 16384, 16384, meters=True)
    eng2.synchronize()


def test_stream_layout_hop(cfg2):
    """Stream layout: overlapping frames of one planar stream via frame_stride = hop."""
    import torch
    from omega_gpu import Engine, Resolution
    W, H, F = 4096, 1024, 16
    s = S.sine(440, 0.25, W + H * (F - 1)) + S.noise(3, W + H * (F - 1), 0.05)
    eng = Engine([Resolution((20, 20000), 4096, 1024, 1.0)], FS, 20000, 256)
    out = eng.process_frames(s, F, H, 0, combined=True, true_peak=True)
    for f in (0, 5, 15):
        fr = s[f * H:f * H + W]
        res = R.mrfft_frame(fr, [R.FFTConfig((20, 20000), 4096, 1024, 1.0)], FS)
        comb, _ = R.combine(res, [R.FFTConfig((20, 20000), 4096, 1024, 1.0)], FS, 20000, 256)
        assert normwise(out["combined"][f], comb) < SPEC_TOL
        assert abs(out["true_peak_db"][f] - R.true_peak(fr)) < TP_TOL_DB
    # omega_process_stream: the same frames from (n_samples, hop); a partial trailing hop is dropped
    eng2 = Engine([Resolution((20, 20000), 4096, 1024, 1.0)], FS, 20000, 256)
    st = eng2.process_stream(s, len(s) - 7, H, combined=True, true_peak=True)
    assert st["combined"].shape == (F - 1, 256)
    np.testing.assert_array_equal(st["combined"], out["combined"][:F - 1])
    np.testing.assert_array_equal(st["true_peak_db"], out["true_peak_db"][:F - 1])
    assert eng2.process_stream(s, W - 1, H)["combined"].shape == (0, 256)


def test_meter_chunks_across_layouts():
    """A batch longer than one meter chunk (kMeterChunk = 2048 frames): the default layout (meter
    prep + LUFS meters on a side stream, the true-peak meter on the main one, chunk by chunk) gives
    the side-meter kernel layout's and the graph path's meters bitwise, and a frame past the chunk boundary matches the oracle's
    sequential calculate_lufs calls."""
    import torch
    from omega_gpu import Engine, Resolution
    from omega_gpu import _lib as L
    W, H, F = 1024, 64, 2100
    n = W + H * (F - 1)
    x = torch.from_numpy(np.stack([S.sine(330, 0.3, n) * (1 + 0.5 * np.sin(np.arange(n) / 9000.0)),
                                   S.noise(5, n, 0.1)]).astype(np.float32).ravel()).cuda()
    res = []
    for flags in (1, 2, 0):  # graphs, direct + side-meter kernels, direct + default
        eng = Engine([Resolution((20, 20000), 1024, 256, 1.0)], FS, 20000, 64, n_channels=2)
        eng._check(L.lib().omega_set_graphs(eng._ctx, flags))
        o = eng.process_stream(x, n, H, channel_stride=n, combined=False, meters=True)
        torch.cuda.synchronize()
        res.append({k: v.cpu().numpy() for k, v in o.items()})
    for r in res[1:]:
        for k in res[0]:
            np.testing.assert_array_equal(res[0][k], r[k], err_msg=k)
    li = res[0]["lufs_inst"].reshape(F, 2)
    tp = res[0]["true_peak_db"].reshape(F, 2)
    st = R.MeterState(FS)
    for f in range(F):
        agg = st.update(np.ones(1), float(li[f, 1]), float(tp[f, 1]))
    np.testing.assert_allclose(res[0]["meters"].reshape(F, 2, 5)[F - 1, 1], list(agg.values()), rtol=0, atol=1e-9)


def test_zero_frames_is_noop():
    from omega_gpu import Engine, Resolution
    e = Engine([Resolution((20, 20000), 1024, 256, 1.0)], FS, 20000, 16)
    out = e.process_frames(np.zeros(1024, np.float32), 0, 1024, 1024)
    assert out["combined"].shape == (0, 16)


def test_graph_replay_matches_direct_launch():
    """Device-memory calls are captured into HIP graphs and replayed; over several consecutive batches
    (meter state ping-pong included) the replayed path equals direct launches of the same kernels and
    the default one-launch batch layout bitwise."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    from omega_gpu import _lib as L
    x = torch.from_numpy(S.cfg2_batch(8)).cuda()
    outs = []
    for flags in (1, 2, 0, 3):
        # graphs (captured: full-chip kernels back to back, meters on a side stream), the same layout on
        # direct launches, direct + default (one batch_kernel launch), graphs with the layout bits set
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        eng._check(L.lib().omega_set_graphs(eng._ctx, flags))
        bufs = [{k: torch.empty(16, *s, dtype=d, device="cuda") for k, s, d in
                 (("combined", (512,), torch.float32), ("lufs_inst", (), torch.float32),
                  ("true_peak_db", (), torch.float32), ("meters", (5,), torch.float64))} for _ in range(2)]
        seq = []
        for i in range(5):
            o = eng.process_frames(x, 8, 2 * 16384, 16384, meters=True, out=bufs[i % 2])
            torch.cuda.synchronize()
            seq.append({k: v.clone() for k, v in o.items()})
        outs.append(seq)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            for k in a:
                assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n_frames", [13, 33])
def test_batch_layout_ragged_and_partial_outputs(n_frames):
    """The default layout (one batch_kernel launch: K-weighting, true-peak / 16384-point pairs, the small
    resolutions; meter prep waiting on the K-weighting count) against the side-meter layout (separate
    kernels, stream events): a channel-frame count that is not a multiple of the 8-frame pair groups,
    per-resolution magnitudes and the weighted signal, subsets of the stages, and meter state carried
    over consecutive calls -- bitwise equal. 13 stereo frames are 8 role groups of segment 0, one period
    of its A B A B B A B A order; 33 are 18 groups, two periods and part of a third (decode_block's
    4 (g >> 3) term), with a last group of 2."""
    import torch
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    from omega_gpu import _lib as L
    x = torch.from_numpy(S.cfg2_batch(n_frames)).cuda()
    calls = [dict(meters=True, mags=True, weighted=True), dict(meters=True), dict(true_peak=False),
             dict(combined=False), dict(lufs=False), dict(meters=True, mags=[0])]
    res = []
    for flags in (0, 6):
        eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
        eng._check(L.lib().omega_set_graphs(eng._ctx, flags))
        seq = []
        for kw in calls:
            o = eng.process_frames(x, n_frames, 2 * 16384, 16384, **kw)
            torch.cuda.synchronize()
            seq.append({k: v.clone() for k, v in o.items()})
        res.append(seq)
    for a, b in zip(*res):
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    # and the first call against the oracle on a few channel-frames
    xn = x.cpu().numpy()
    out = {k: v.cpu().numpy() for k, v in res[0][0].items()}
    for f, c in ((0, 0), (6, 1), (12, 1)):
        _, comb, li, tp = R.full_frame(xn[f, c])
        cf = 2 * f + c
        assert normwise(out["combined"][cf], comb) < SPEC_TOL
        assert abs(out["lufs_inst"][cf] - li) < LU_TOL
        assert abs(out["true_peak_db"][cf] - tp) < TP_TOL_DB


def test_spectra_cfg3_vs_oracle():
    """cfg3 fused analysis (omega_spectra): Hann rfft magnitude (A13) -> 512 log bands (A10) and the
    raw chromagram (A12) of alternating triad / noise frames, against the oracle chain. Tolerances:
    magnitudes 1e-4 normwise (north star), bands 1e-4 relative, chroma 1e-5 relative (float32
    projection weights instead of the reference's float64 matrix). The 1e-4 is the north-star bar only: the
    float32-accuracy comparison of the magnitudes, bin by bin on designed signals, is
    tests/test_pow2_rfft_bins.py (test_spectra_rf)."""
    from omega_gpu import Engine, Resolution
    from omega_gpu.engine import BandTable
    from omega_gpu import _lib as L
    x = S.cfg3_batch(16)
    eng = Engine([Resolution((20, 20000), 8192, 2048, 1.0)], FS, 20000, 512)
    st, en, comp = R.pipeline_band_table(FS, 512, 8192)
    bt = BandTable(eng, L.BANDS_MAX, st, en, 512, 4097, scale=comp)
    out = eng.spectra(x, "hann", bands=bt, chroma=True, mags=True)
    freqs = np.fft.rfftfreq(8192, 1 / FS)
    for f in range(len(x)):
        mag = R.batched_fft(x[f], 8192, "hann")["magnitude"]
        assert normwise(out["mag"][f], mag) < SPEC_TOL
        bands = R.map_to_bands(mag.astype(np.float32), st, en, comp, 512)
        np.testing.assert_allclose(out["bands"][f], bands, rtol=1e-4, atol=1e-6 * np.max(bands))
        ch = R.ChromaState().compute(mag.astype(np.float32), freqs)
        np.testing.assert_allclose(out["chroma"][f], ch, rtol=1e-5, atol=1e-9)
    # the band stage equals the standalone A10 entry point on the same magnitudes
    np.testing.assert_array_equal(out["bands"], bt.apply(out["mag"]))


def test_spectra_cfg3_full_batch():
    """The launch bench.py's cfg3 line times: 4096 frames x 8192 in one omega_spectra call (bands with
    the compensation scale + chromagram, device input, no magnitudes). Every output finite, bands and
    chroma non-negative, chroma normalised (sum 1 on every frame with energy); all 4096 frames' bands
    and chroma against the oracle chain."""
    import torch
    from omega_gpu import Engine, Resolution
    from omega_gpu.engine import BandTable
    from omega_gpu import _lib as L
    n = 4096
    x = S.cfg3_batch(n)
    eng = Engine([Resolution((20, 20000), 8192, 2048, 1.0)], FS, 20000, 512)
    st, en, comp = R.pipeline_band_table(FS, 512, 8192)
    bt = BandTable(eng, L.BANDS_MAX, st, en, 512, 4097, scale=comp)
    xd = torch.from_numpy(x).cuda()
    out = eng.spectra(xd, "hann", bands=bt, chroma=True)
    torch.cuda.synchronize()
    bands, chroma = out["bands"].cpu().numpy(), out["chroma"].cpu().numpy()
    assert bands.shape == (n, 512) and chroma.shape == (n, 12)
    assert np.isfinite(bands).all() and np.isfinite(chroma).all()
    assert (bands >= 0).all() and (chroma >= 0).all()
    np.testing.assert_allclose(chroma.sum(axis=1), 1.0, rtol=1e-12)
    # every frame's bands and chroma against the whole-batch oracle (omega_ref.spectra_batch, pinned
    # to the per-frame chain on the CPU)
    _, want_b, want_c = R.spectra_batch(x, st, en, comp, 512)
    for f in range(n):
        np.testing.assert_allclose(bands[f], want_b[f], rtol=1e-4, atol=1e-6 * np.max(want_b[f]), err_msg=f"frame {f}")
    np.testing.assert_allclose(chroma, want_c, rtol=1e-5, atol=1e-9)


def test_cfg1_stream_momentary_lufs():
    """BASELINE cfg1 (configs[0]): one 48 kHz mono stream, hop 512, W = 1024, one 1024-point
    resolution, 600 frames of 0.5 sin(2 pi 1000 t): the combined spectrum, LUFS_inst and the meter
    aggregates (momentary over the last 24 frames) of every frame against the oracle's per-frame loop
    (calculate_lufs fed frame by frame)."""
    from omega_gpu import Engine, Resolution
    W, H, F = 1024, 512, 600
    n = W + H * (F - 1)
    x = S.sine(1000, 0.5, n)
    eng = Engine([Resolution((20, 20000), W, H, 1.0)], FS, 20000, target_bins=512, frame_size=W)
    out = eng.process_stream(x, n, H, combined=True, meters=True)
    assert out["lufs_inst"].shape == (F,)
    st = R.MeterState(FS)
    cfgs = (R.FFTConfig((20, 20000), W, H, 1.0),)
    for f in range(F):
        fr = x[f * H:f * H + W]
        _, comb, li, tp = R.full_frame(fr, configs=cfgs, target_bins=512)
        assert normwise(out["combined"][f], comb) < SPEC_TOL, f
        assert abs(out["lufs_inst"][f] - li) < LU_TOL, f
        assert abs(out["true_peak_db"][f] - tp) < TP_TOL_DB, f
        agg = st.update(fr, li, tp)
        assert abs(out["meters"][f][0] - agg["momentary"]) < LU_TOL, f
        assert abs(out["meters"][f][1] - agg["short_term"]) < LU_TOL, f
        assert abs(out["meters"][f][4] - agg["true_peak"]) < TP_TOL_DB, f


def test_cfg5_stream_96k_surround():
    """BASELINE cfg5 shape at small size: 96 kHz, 8 channels, stream layout (hop 1024) of 16384-point
    frames with true peak, K-weighted LUFS (filters designed for 96 kHz) and the meter aggregates,
    against the oracle per channel (a few frames of each channel's stream)."""
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    fs, C, W, H, F = 96000, 8, 16384, 1024, 6
    n = W + H * (F - 1)
    t = np.arange(n) / fs
    x = np.stack([(0.2 * np.sin(2 * np.pi * 110 * (c + 1) * t)).astype(np.float32) +
                  S.noise(c, n, 0.02) for c in range(C)]).astype(np.float32)
    eng = Engine(NORTHSTAR_RESOLUTIONS, fs, 20000, target_bins=512, n_channels=C)
    out = eng.process_stream(x.ravel(), n, H, channel_stride=n, combined=True, meters=True)
    assert out["lufs_inst"].shape == (F * C,)
    for c in (0, 3, 7):
        st = R.MeterState(fs)
        for f in range(F):
            fr = x[c, f * H:f * H + W]
            _, comb, li, tp = R.full_frame(fr, fs=fs)
            cf = f * C + c
            assert normwise(out["combined"][cf], comb) < SPEC_TOL
            assert abs(out["lufs_inst"][cf] - li) < LU_TOL
            assert abs(out["true_peak_db"][cf] - tp) < TP_TOL_DB
            agg = np.array(list(st.update(fr, li, tp).values()))
            assert np.all(np.abs(out["meters"][cf][:4] - agg[:4]) < LU_TOL)
            assert abs(out["meters"][cf][4] - agg[4]) < TP_TOL_DB


# ---- drum-detection features (omega_drum_features) ----
# Fluxes are float32 sums as in the reference, but summed in another order (numpy: pairwise; here:
# per-thread runs + a tree): relative 1e-5 on fluxes and thresholds; the centroid is float64.
DRUM_RTOL = 1e-5


def _drum_close(got, want):
    scale = np.maximum(np.abs(want), 1e-3 * np.max(np.abs(want), axis=0, keepdims=True) + 1e-12)
    return np.max(np.abs(got - want) / scale)


@pytest.mark.parametrize("name", ["drums_1025", "drums_2049"])
def test_drum_features_golden(name):
    """The reference's EnhancedKickDetector / EnhancedSnareDetector outputs (golden) and the oracle's
    snare thresholds, frame by frame over one stream, from one call."""
    from omega_gpu.drum_detection import DrumFeatures
    g = load_golden("drums")
    mags, ref = g[f"{name}/mags"], g[f"{name}/out"]
    out = DrumFeatures(FS).process(mags)
    assert out.shape == (len(mags), 14) and out.dtype == np.float64
    assert _drum_close(out[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13]], ref) < DRUM_RTOL
    assert _drum_close(out, R.drum_sequence(mags)) < DRUM_RTOL


def test_drum_features_state_across_calls_and_device_input():
    """Calls of 1, 7 and the rest of the frames continue one stream (previous frame, histories);
    device tensors with a padded row stride give the same; reset starts a new stream; a stream's bin
    count is fixed."""
    import torch
    from omega_gpu import Engine, OmegaError
    from omega_gpu.drum_detection import DrumFeatures
    mags = load_golden("drums")["drums_1025/mags"]
    whole = DrumFeatures(FS).process(mags)
    d = DrumFeatures(FS)
    parts = np.concatenate([d.process(mags[:1]), d.process(mags[1:8]), d.process(mags[8:])])
    assert _drum_close(parts, whole) < DRUM_RTOL
    d.reset()
    np.testing.assert_array_equal(d.process(mags), whole)
    eng = Engine(sample_rate=FS)
    padded = torch.zeros(len(mags), 1040, device="cuda")
    padded[:, :1025] = torch.from_numpy(mags).cuda()
    o = eng.drum_features(padded[:, :1025])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(o.cpu().numpy(), whole)
    with pytest.raises(OmegaError):
        eng.drum_features(np.zeros((2, 513), np.float32))
    assert eng.drum_features(np.zeros((0, 1025), np.float32)).shape == (0, 14)


def test_drum_features_random_vs_oracle():
    """Random magnitudes over a long stream (past the 21-deep history, several calls), sensitivity 1.5."""
    from omega_gpu.drum_detection import DrumFeatures
    rng = np.random.default_rng(11)
    mags = np.abs(rng.standard_normal((70, 2049))).astype(np.float32) * np.linspace(2, 0.1, 2049).astype(np.float32)
    d = DrumFeatures(FS, sensitivity=1.5)
    got = np.concatenate([d.process(mags[:33]), d.process(mags[33:])])
    assert _drum_close(got, R.drum_sequence(mags, FS, 1.5)) < DRUM_RTOL


POST_CFG = {"default": ({}, {}),
            "vocal_supp_norm": (dict(vocal_suppression=0.4, normalization=True),
                                dict(vocal_suppression=0.4, normalization_enabled=True)),
            "flat": (dict(psycho=False, freq_comp=False, smoothing=False),
                     dict(psychoacoustic_enabled=False, freq_compensation_enabled=False, smoothing_enabled=False))}
@pytest.mark.parametrize("name", sorted(POST_CFG))
def test_app_post_golden(name):
    """The app's own post-processing (golden, gen_golden.gen_post) from its combined spectra: spectrum,
    content types and band values bit-exact."""
    from omega_gpu.app_post import SpectrumPostProcessor
    g = load_golden("app_post")
    pp = SpectrumPostProcessor(g[f"{name}/freqs"], **POST_CFG[name][1])
    s, b, c = pp.process(g[f"{name}/combined"])
    np.testing.assert_array_equal(s, g[f"{name}/spectrum"])
    np.testing.assert_array_equal(c, g[f"{name}/content"])
    np.testing.assert_array_equal(b, g[f"{name}/bands"])


def _post_ema_input(g):
    c = np.zeros((int(g["n_frames"]), g["combined"].shape[1]), np.float32)
    c[:len(g["combined"])] = g["combined"]
    return c


def test_app_post_ema_through_silence_golden():
    """The reference's own loop over 1000 note frames and 500 silent ones (gen_golden.gen_post_ema):
    band values bit-exact through the silence -- the bands keep decaying into float32 denormals where a
    chunk warmed up from silent frames alone would sit at 0 -- in one 1500-frame call (24 EMA chunks)
    and in calls of 1, 63, 700 and the rest."""
    from omega_gpu.app_post import SpectrumPostProcessor
    g = load_golden("post_ema")
    x = _post_ema_input(g)
    pp = SpectrumPostProcessor(g["freqs"])
    s, b, c = pp.process(x)
    np.testing.assert_array_equal(b, g["bands"])
    np.testing.assert_array_equal(c, g["content"])
    assert (b[-1] < 1e-30).all() and (b[-1] > 0).sum() > 400
    pp.reset()
    parts = [pp.process(x[a:e])[1] for a, e in ((0, 1), (1, 64), (64, 764), (764, len(x)))]
    np.testing.assert_array_equal(np.concatenate(parts), g["bands"])


def test_app_post_ema_slow_factors_exact():
    """EMA factors up to 0.995 (the warm-up no longer fades out within a chunk's 256-frame lead: the
    fix pass re-runs those chunks) give the sequential recurrence bit for bit in one 900-frame call."""
    import omega_gpu.app_post as AP
    g = load_golden("app_post")
    freqs = g["default/freqs"]
    rng = np.random.default_rng(17)
    x = (rng.random((900, 512)) * rng.random((900, 1)) ** 2).astype(np.float32)
    x[300:700] = 0.0
    orig_dev, orig_ref = AP._band_table, R.app_band_table

    def slow_dev(*a):
        bs, be, f = orig_dev(*a)
        return bs, be, np.linspace(0.9, 0.995, len(f))

    def slow_ref(*a):
        keep, f = orig_ref(*a)
        return keep, [float(v) for v in np.linspace(0.9, 0.995, len(f))]  # Python floats, as the app's
    try:
        AP._band_table, R.app_band_table = slow_dev, slow_ref
        _, b, _ = AP.SpectrumPostProcessor(freqs).process(x)
        _, wb, _ = R.app_post_sequence(x, freqs)
    finally:
        AP._band_table, R.app_band_table = orig_dev, orig_ref
    np.testing.assert_array_equal(b, wb)


def test_app_post_ema_chunk_groups_exact():
    """One 5000-frame call (79 EMA chunks: the boundary checks and re-runs go in groups of 64 chunks)
    with a 800-frame silence across the group boundary at frame 4096, where the decaying bands make
    every warmed-up chunk re-run and the rewritten chunk ends carry into the next group: equal bit for
    bit to the same frames in single-frame calls (each one the plain sequential step, golden-tested)."""
    from omega_gpu.app_post import SpectrumPostProcessor
    freqs = load_golden("app_post")["default/freqs"]
    rng = np.random.default_rng(23)
    x = (rng.random((5000, 512)) * rng.random((5000, 1)) ** 2).astype(np.float32)
    x[3800:4600] = 0.0
    pp = SpectrumPostProcessor(freqs)
    _, b, c = pp.process(x)
    pp.reset()
    seq = np.concatenate([pp.process(x[f:f + 1])[1] for f in range(len(x))])
    np.testing.assert_array_equal(b, seq)
    assert (b[4599] > 0).sum() > 100  # (still decaying at the end of the silence)


def test_app_post_content_threshold_frames():
    """Frames whose bass ratio sits within a few ulps of the 0.6 threshold, where float64 range sums
    and numpy's float32 pairwise np.mean disagree (tests/golden/gen_post_threshold.py): the device
    classifies as the reference does."""
    from omega_gpu.app_post import SpectrumPostProcessor
    g = np.load(os.path.join(GOLDEN, "post_threshold.npz"))  # labels: the reference's update_content_type
    assert (g["content"] != g["content_f64"]).all()
    freqs = load_golden("app_post")["default/freqs"]
    pp = SpectrumPostProcessor(freqs, psychoacoustic_enabled=False, freq_compensation_enabled=False)
    s, b, c = pp.process(g["combined"])
    np.testing.assert_array_equal(c, g["content"])
    ws, wb, wc = R.app_post_sequence(g["combined"], freqs, psycho=False, freq_comp=False)
    np.testing.assert_array_equal(s, ws)


def test_app_post_nan_frame():
    """A NaN in a frame: numpy's max/percentile give NaN, so the frame is not normalised and the
    content type is instrumental; the other frames are unaffected."""
    from omega_gpu.app_post import SpectrumPostProcessor
    freqs = load_golden("app_post")["default/freqs"]
    rng = np.random.default_rng(9)
    x = rng.random((3, 512)).astype(np.float32)
    x[1, 100] = np.nan
    pp = SpectrumPostProcessor(freqs, smoothing_enabled=False)
    s, b, c = pp.process(x)
    with np.errstate(invalid="ignore"):
        ws, wb, wc = R.app_post_sequence(x, freqs, smoothing=False)
    np.testing.assert_array_equal(s, ws)
    np.testing.assert_array_equal(c, wc)


def test_app_post_percentile_ties_and_zeros():
    """The 98th percentile by radix select over the float order keys: spectra with heavy ties
    (quantised values), runs of zeros (+0 and -0), negative values, a frame whose top 3 % are equal,
    1024-bin frames (radix select) and 512-, 300- and 40-bin frames (the per-wave top-16 sort; at 40
    bins the vocal and high ranges are empty: numpy's NaN means), bitwise against the oracle
    (np.percentile)."""
    from omega_gpu.app_post import SpectrumPostProcessor
    rng = np.random.default_rng(13)
    for T in (512, 1024, 300, 40):
        freqs = np.linspace(0, 20000, T)
        F = 12
        x = (np.round(rng.random((F, T)) * 8) / 8).astype(np.float32)  # 9 distinct values
        x[0, : T // 2] = 0.0
        x[1, ::2] = -0.0
        x[2] = np.float32(0.25)
        x[2, -T // 32:] = np.float32(3.0)                                # top 3 % equal
        x[3] = rng.standard_normal(T).astype(np.float32)                 # negative values
        x[4, :-1] = 0.0
        x[5] = np.arange(T, dtype=np.float32)[::-1]
        pp = SpectrumPostProcessor(freqs, smoothing_enabled=False)
        sp, b, c = pp.process(x)
        with np.errstate(invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ws, wb, wc = R.app_post_sequence(x, freqs, smoothing=False)
        np.testing.assert_array_equal(sp, ws, err_msg=f"T={T}")
        np.testing.assert_array_equal(c, wc)


def test_app_post_random_state_and_device_input():
    """Random spectra (every content branch) against the oracle; calls of 1, 9 and the rest continue
    the band EMA; device input with a padded row stride; reset starts a new stream."""
    import torch
    from omega_gpu.app_post import SpectrumPostProcessor
    g = load_golden("app_post")
    freqs = g["default/freqs"]
    rng = np.random.default_rng(5)
    F = 40
    x = (rng.random((F, 512)) * rng.random((F, 1)) ** 2).astype(np.float32)
    x[::3, :6] *= 40.0      # bass-heavy frames
    x[1::3, :8] *= 0.01     # vocal-range frames
    x[1::3, 8:85] *= 8.0
    x[2::3, :8] *= 0.01     # treble-heavy frames: instrumental
    x[2::3, 128:] *= 10.0
    x[5] = 0.0              # silent frame: no normalisation, instrumental
    ws, wb, wc = R.app_post_sequence(x, freqs, vocal_suppression=0.2)
    assert set(wc.tolist()) == {0, 1, 2}
    pp = SpectrumPostProcessor(freqs, vocal_suppression=0.2)
    s, b, c = pp.process(x)
    np.testing.assert_array_equal(s, ws)
    np.testing.assert_array_equal(c, wc)
    np.testing.assert_array_equal(b, wb)
    pp.reset()
    xd = torch.zeros((F, 640), dtype=torch.float32, device="cuda")
    xd[:, :512] = torch.from_numpy(x).cuda()
    xd = xd[:, :512]
    parts = [pp.process(xd[a:e]) for a, e in ((0, 1), (1, 10), (10, F))]
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.cat([p[0] for p in parts]).cpu().numpy(), s)
    np.testing.assert_array_equal(torch.cat([p[1] for p in parts]).cpu().numpy(), b)


def test_app_post_ema_chunks_join_the_sequential_recurrence():
    """700 frames in one call (the band EMA runs as 11 chunks of 64 frames, the later ones warmed up
    over the 256 frames before them and checked against the sequential state) give bit for bit the
    bands of 7 sequential calls of 100 frames, and the oracle's."""
    from omega_gpu.app_post import SpectrumPostProcessor
    freqs = load_golden("app_post")["default/freqs"]
    rng = np.random.default_rng(12)
    x = (rng.random((700, 512)) * rng.random((700, 1)) ** 2).astype(np.float32)
    s1, b1, c1 = SpectrumPostProcessor(freqs).process(x)
    pp = SpectrumPostProcessor(freqs)
    parts = [pp.process(x[i:i + 100]) for i in range(0, 700, 100)]
    np.testing.assert_array_equal(b1, np.concatenate([p[1] for p in parts]))
    np.testing.assert_array_equal(s1, np.concatenate([p[0] for p in parts]))
    ws, wb, wc = R.app_post_sequence(x, freqs)
    np.testing.assert_array_equal(b1, wb)
